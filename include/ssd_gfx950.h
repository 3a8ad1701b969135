/*
 * ssd_gfx950.h -- C ABI of libssd_gfx950.so: the MI355X (gfx950) SSD300 hot path.
 *
 * The reference (nitishsaDire/objectDetection_ssd) has no native layer: its hot
 * path is Python calling ATen ops.  This header is the boundary a maintainer
 * binds instead (ctypes stub in INTEGRATION.md).  Every entry point names the
 * reference call site it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers + sizes, no framework types; all pointers are DEVICE
 *     pointers unless a parameter is documented as host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - functions only enqueue work: they never allocate, synchronise or throw;
 *   - return 0 on success or a negative ssd_status code;
 *   - activations are NHWC f32; "packed" head buffers are [N*H*W][ld] f32.
 */
#ifndef SSD_GFX950_H
#define SSD_GFX950_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSD_ABI_VERSION 1

enum ssd_status {
    SSD_OK = 0,
    SSD_ERR_BAD_SHAPE = -1,   /* unsupported / inconsistent dimensions            */
    SSD_ERR_WORKSPACE = -2,   /* workspace too small                              */
    SSD_ERR_NULL = -3,        /* required pointer is NULL                         */
    SSD_ERR_LAUNCH = -4,      /* hipGetLastError() != hipSuccess after enqueue    */
    SSD_ERR_ALIGN = -5        /* pointer / leading dimension not 16-byte aligned  */
};

int ssd_abi_version(void);
const char* ssd_status_string(int status);

/* Geometry of one convolution, forward sense.  (torch.nn.Conv2d arguments of
 * Model.py:135-184: kernel R x S, stride, padding, dilation.) */
typedef struct ssd_conv_geom {
    int32_t N, H, W, Ci;      /* input  NHWC                                     */
    int32_t Ho, Wo, Co;       /* output NHWC                                     */
    int32_t R, S;             /* taps                                            */
    int32_t stride, pad, dil;
} ssd_conv_geom;

/* ---- weight layouts --------------------------------------------------------
 * nn.Conv2d keeps OIHW.  The kernels read K-contiguous rows:
 *   forward : [Co_pad][R*S][Ci]   (rows >= Co zero)
 *   dgrad   : [Ci][R*S][Co_pad]   (columns >= Co zero)
 * Replaces nothing in the reference (ATen re-lays weights internally). */
int ssd_weight_oihw_to_ohwi(const float* w_oihw, float* w_ohwi, int Co, int Ci, int R, int S, int Co_pad, void* stream);
int ssd_weight_oihw_to_ihwo(const float* w_oihw, float* w_ihwo, int Co, int Ci, int R, int S, int Co_pad, void* stream);

/* ---- convolution (Model.py:135-184 nn.Conv2d + nn.ReLU; autograd of them,
 * train_function.py:94) ------------------------------------------------------
 * y[m][n] = act( sum_{tap,c} x[pix(m,tap)][c] * w[n][tap][c] + bias[n] ),  m = (n,ho,wo).
 * Ci % 32 == 0 required (conv1_1 has its own entry below).  ldy = row stride of y
 * in floats (>= Co).  relu: 0/1. */
int ssd_conv2d_fwd(const float* x, const float* w_ohwi, const float* bias, float* y, int ldy,
                   const ssd_conv_geom* g, int relu, void* stream);

/* dx[pix][c] (+)= sum_{tap,n} dy[opix(pix,tap)][n] * w[n][c][tap];  then, if
 * relu_mask != NULL, dx = relu_mask > 0 ? dx : 0 (relu_mask = the post-ReLU
 * activation that produced x).  dy rows have stride ldy (>= Co_pad, pad columns
 * zero), Co_pad % 32 == 0. */
int ssd_conv2d_dgrad(const float* dy, int ldy, const float* w_ihwo, int Co_pad, float* dx,
                     const float* relu_mask, int accumulate, const ssd_conv_geom* g, void* stream);

/* bf16-operand variants (BASELINE.json configs[2] "bf16 convs"): identical signatures and f32 tensors; the
 * operand tiles are rounded to bf16 on their way into LDS and multiplied on v_mfma_f32_32x32x16_bf16 with f32
 * accumulation.  Opt-in (Model.SSD_300.conv_dtype = "bf16").  The weight gradient has a bf16 kernel for the 3x3 / stride 1
 * layers on maps >= 30 px (same workspace query as the f32 entry); other layers fall through to the f32 kernels. */
int ssd_conv2d_fwd_bf16(const float* x, const float* w_ohwi, const float* bias, float* y, int ldy,
                        const ssd_conv_geom* g, int relu, void* stream);
int ssd_conv2d_dgrad_bf16(const float* dy, int ldy, const float* w_ihwo, int Co_pad, float* dx,
                          const float* relu_mask, int accumulate, const ssd_conv_geom* g, void* stream);
/* ... with the split-K workspace of ssd_conv2d_igemm_workspace(g, direction) (may be NULL): small grids with a deep K loop -- the 10x10 ... 1x1
 * maps of the aux blocks and heads -- are cut into K slices, reduced in slice order (reproducible) */
int ssd_conv2d_fwd_bf16_ws(const float* x, const float* w_ohwi, const float* bias, float* y, int ldy, const ssd_conv_geom* g, int relu,
                           void* workspace, size_t workspace_bytes, void* stream);
int ssd_conv2d_dgrad_bf16_ws(const float* dy, int ldy, const float* w_ihwo, int Co_pad, float* dx, const float* relu_mask, int accumulate,
                             const ssd_conv_geom* g, void* workspace, size_t workspace_bytes, void* stream);
int ssd_conv2d_wgrad_bf16(const float* x, const float* dy, int ldy, float* dw_oihw, float* dbias,
                          const ssd_conv_geom* g, void* workspace, size_t workspace_bytes, void* stream);
int ssd_tune_set_igemm_bf16(int tile);   /* 0 = 256x128, 1 = 128x128, 2 = 128x64, 3 = 64x64, -1 = automatic */

/* "f32 from three bf16 limbs" variants (opt-in: Model.SSD_300.conv_dtype = "f32x3"): every operand is split exactly
 * into hi + mid + lo bf16 limbs (8+8+8 significant bits); a product block is the six limb products of weight >= 2^-16
 * on the bf16 MFMA with f32 accumulation (dropped terms <= 2^-24 relative).  Weights are passed pre-split:
 * ssd_weight_split_bf16x3 writes three bf16 planes [3][n] from an f32 array of n elements (the OHWI / IHWO layouts
 * above); w_rows = rows of the OHWI layout (>= Co). */
int ssd_weight_split_bf16x3(const float* w, void* planes_bf16, size_t n, void* stream);
int ssd_conv2d_fwd_x3(const float* x, const void* w3_ohwi, int w_rows, const float* bias, float* y, int ldy,
                      const ssd_conv_geom* g, int relu, void* stream);
int ssd_conv2d_dgrad_x3(const float* dy, int ldy, const void* w3_ihwo, int Co_pad, float* dx,
                        const float* relu_mask, int accumulate, const ssd_conv_geom* g, void* stream);
int ssd_tune_set_igemm_x3(int tile);     /* 1 = 128x128, 2 = 128x64, 3 = 64x64, -1 = automatic */
/* bf16-operand halo-tile kernels for 3x3/s1/p1 layers (plane 0 of the split weights); return 1 (not an error) when the
 * geometry is not a halo case and the caller should use the generic bf16 entry. */
int ssd_conv3x3_halo_fwd_bf16(const float* x, const void* w3_ohwi, int w_rows, const float* bias, float* y, int ldy,
                              const ssd_conv_geom* g, int relu, void* stream);
int ssd_conv3x3_halo_dgrad_bf16(const float* dy, int ldy, const void* w3_ihwo, int Co_pad, float* dx,
                                const float* relu_mask, int accumulate, const ssd_conv_geom* g, void* stream);
int ssd_tune_set_halo(int mode);         /* 3x3/s1 halo-tile kernel: 0 = off, 1 = 8x8 patches, 2 = 8x16 patches, -1 = automatic */

/* ---- bf16 TENSORS (round 3; BASELINE.json configs[2] "bf16 convs" with activations and gradients stored in bf16) ------------
 * 3x3 / stride 1 / pad 1 convolution, forward (flip = 0) and data gradient (flip = 1: the same convolution with the taps
 * mirrored), replacing nn.Conv2d(+ReLU) of Model.py:135-143,176-184 and its autograd data gradient.
 *   x        [N][H][W][ldx] bf16 (forward: the input activation; data gradient: dy), K = reduction channels per tap (multiple of 64, <= ldx)
 *   w        [w_rows][9][K] bf16 (forward: OHWI copy of the f32 master; data gradient: IHWO); rows >= w_rows count as zero
 *   out      [N][H][W][ldo] bf16, or f32 when out_f32 (the heads): columns 0 .. n_out-1 are written (n_out % 4 == 0; bias, if given, has w_rows entries)
 *   out = [accumulate: out +] conv (+ bias) -> [relu] -> [relu_mask (bf16, out's layout): kept where mask > 0]
 * f32 accumulation on v_mfma_f32_32x32x16_bf16, one rounding to bf16 at the store. */
int ssd_conv3x3_bf16(const void* x, int ldx, const void* w, int w_rows, int K, const float* bias, void* out, int ldo, int n_out,
                     int out_f32, const void* relu_mask, int accumulate, int relu, int flip, int N, int H, int W, void* stream);
int ssd_tune_set_conv_bf16_mfma(int rows);        /* MFMA shape of the bf16-tensor convolution kernels: 32 (32x32x16, default) or 16 (16x16x32) */
int ssd_tune_set_conv_bf16_k64(int on);          /* 0 = K = 64 / <= 64-channel launches on the general kernel instead of the persistent one */
int ssd_tune_set_conv_bf16(int mode, int bn);    /* position space 0 / 1 / 2 (patches 8x32, 16x16, flat), N tile 64 / 128; -1 = automatic */
/* Weight gradient of a 3x3 / stride 1 / pad 1 / dilation 1 layer from bf16 x (N,H,W,Ci) and bf16 dy (N,H,W,ldy): dw (Co,Ci,3,3) and dbias
 * in f32 (the fused nine-tap bf16 MFMA kernel; workspace ssd_conv2d_wgrad_workspace(g)); SSD_ERR_BAD_SHAPE for other geometries. */
int ssd_conv3x3_wgrad_bf16t(const void* x_bf16, const void* dy_bf16, int ldy, float* dw_oihw, float* dbias, const ssd_conv_geom* g,
                            void* workspace, size_t workspace_bytes, void* stream);
/* conv1_1 (Model.py:135) in the bf16-tensor mode: x (f32 NCHW image) and the filter rows rounded to bf16, f32 accumulate, y stored as
 * bf16 NHWC; its weight gradient from the f32 image and the bf16 dy (f32 arithmetic). */
int ssd_conv1_first_fwd_bf16(const float* x_nchw, const float* w_rows, const float* bias, void* y_nhwc_bf16, int N, int H, int W, int relu,
                             void* stream);
int ssd_conv1_first_wgrad_bf16(const float* x_nchw, const void* dy_nhwc_bf16, float* dw_rows, float* dbias, int N, int H, int W,
                               void* workspace, size_t workspace_bytes, void* stream);
/* Max pooling (Model.py:135-142), conv4_3 L2 normalisation (Model.py:206-209) and the heads' gradient gather on bf16 NHWC tensors
 * (C % 8 == 0; argmax codes as in ssd_maxpool_fwd; f32 arithmetic, one rounding at the store; the L2 norm's backward carries its two row sums and dx, whose two
 * terms cancel, in f64, so that dx is the exact value rounded).  ssd_maxpool_bwd_bf16: relu_mask (the bf16
 * activation, dx kept where > 0) and accumulate, or y_gate (the bf16 pooled output: the gated form, no accumulate).
 *
 * REFUSALS of the pool, L2-norm, head, cast and channel_affine entries, f32 and bf16 alike.  Each is made before anything is enqueued,
 * and where several apply the first of this list is returned:
 *   1. SSD_ERR_NULL       a required pointer is NULL (optional: the forward's argmax, relu_mask, the bf16 backward's y_gate);
 *   2. SSD_ERR_BAD_SHAPE  a count (N, H, W, C, Ho, Wo, M, HW, A, n_classes, n) <= 0; C no multiple of the vector (4 channels in f32 and in
 *                         channel_affine, 8 in bf16; 512 exactly for the L2 norm; n % 8 for the casts); k outside 1..15, stride <= 0, pad < 0;
 *                         in the pool forward also 2*pad > k and a last window that lies wholly outside the input
 *                         ((Ho-1)*stride - pad >= H, the same for W); y_gate together with relu_mask or accumulate; heads: ld below
 *                         A*(4+n_classes), prior_off < 0, prior_off + HW*A > P;
 *   3. SSD_ERR_ALIGN      a tensor, gamma, scale, shift, a given relu_mask or y_gate not 16-byte aligned; given argmax codes not aligned to
 *                         one thread's codes (4 bytes in f32, 8 in bf16).  The heads' buffers are accessed by element: no alignment rule;
 *   4. SSD_ERR_WORKSPACE  workspace_bytes below the entry's query.
 * The other entries of the same two source files -- the weight re-layouts, ssd_im2col_first, ssd_im2col_nchw3, ssd_clock_probe,
 * ssd_graph_node_counts, ssd_sgd_momentum(_guarded) -- refuse in the same order: a NULL required pointer (grad_scale_dev is optional); then
 * a count <= 0, Co_pad < Co, pad < 0, Kpad no multiple of 4 or below R*S*3, Ho / Wo that are not the convolution's; then an im2col `out`
 * that is not 16-byte aligned.  The SGD entries take n == 0 as SSD_OK. */
int ssd_maxpool_fwd_bf16(const void* x, void* y, uint8_t* argmax, int N, int H, int W, int C, int k, int stride, int pad, int Ho, int Wo,
                         void* stream);
int ssd_maxpool_bwd_bf16(const void* dy, const uint8_t* argmax, void* dx, const void* relu_mask, const void* y_gate, int accumulate, int N,
                         int H, int W, int C, int k, int stride, int pad, int Ho, int Wo, void* stream);
int ssd_l2norm_fwd_bf16(const void* x, const float* gamma, void* y, int M, int C, void* stream);
size_t ssd_l2norm_bwd_bf16_workspace(int M, int C);
int ssd_l2norm_bwd_bf16(const void* x, const float* gamma, const void* dy, void* dx, float* dgamma, int M, int C, void* workspace,
                        size_t workspace_bytes, void* stream);
int ssd_heads_gather_bf16(const float* dloc, const float* dconf, void* packed_bf16, int ld, int N, int HW, int A, int prior_off, int P,
                          int ncls, void* stream);
/* n % 8 == 0.  f32 -> bf16 rounds to nearest even over the whole range -- ties, f32 and bf16 subnormals, overflow to inf -- and keeps a
 * NaN a NaN; bf16 -> f32 is exact, bit for bit. */
int ssd_cast_f32_bf16(const float* x, void* y_bf16, size_t n, void* stream);
int ssd_cast_bf16_f32(const void* x_bf16, float* y, size_t n, void* stream);
/* ssd_weights_prepare job kind 3: out_fwd = bf16 OHWI [co_pad][taps][ci], out_bwd = bf16 IHWO [ci][taps][pad1] (pad1 >= co, zero filled). */

/* dw_oihw[n][c][r][s] = sum_m dy[m][n] * x[pix(m,tap)][c];  dbias[n] = sum_m dy[m][n]
 * (dbias may be NULL).  Deterministic: split-K partial slabs in `workspace`, then a
 * fixed-order reduction. */
size_t ssd_conv2d_wgrad_workspace(const ssd_conv_geom* g);
int ssd_conv2d_wgrad(const float* x, const float* dy, int ldy, float* dw_oihw, float* dbias,
                     const ssd_conv_geom* g, void* workspace, size_t workspace_bytes, void* stream);

/* Introspection for profiling: which tile configuration the dispatcher picks (direction 0 = forward,
 * 1 = dgrad), and the wgrad tile edge / split-K factor.  Used by bench.py to attribute HIP-event
 * timings to kernel instantiations; no effect on results. */
int ssd_conv2d_igemm_tile(const ssd_conv_geom* g, int direction, int* bm, int* bn);
int ssd_conv2d_wgrad_tile(const ssd_conv_geom* g, int* bt, int* nsplit);
/* Host-only plan queries (no GPU needed); each reports what the entry point launches under the current tuning aids, from the same function
 * the dispatcher calls.
 * ssd_conv2d_wgrad_plan: plan[8] = kernel (0 one tap per block, 1 f32 nine-tap, 2 bf16 patch kernel), tile edge, LDS stages, f32 nine-tap
 *   patch shape (0 = 4x8, 1 = 1x38, 2 = 2x19; -1 otherwise), bf16 patch form (0 = 3x3, 1 = dilation 4, 2 = 1x1; -1 otherwise), nsplit,
 *   positions (or patches) per split, slab reduction (1 = one block per tap, 0 = per output channel and 64 input channels); bf16 selects
 *   ssd_conv2d_wgrad_bf16 / ssd_conv3x3_wgrad_bf16t (the latter takes bf16 patch-kernel plans only).
 * ssd_conv3x3_bf16_plan: plan[4] = position space (0 = 8x32 patches, 1 = 16x16, 2 = flat), N tile (64 / 128), halo pieces per wave,
 *   persistent K = 64 kernel (0 / 1) of ssd_conv3x3_bf16 on an N x H x W map with K input and n_out output channels.
 * ssd_conv3x3_halo_shape: the halo kernel's patch shape for a forward (direction 0) or data gradient (1) with 1 (bf16-operand) or 3
 *   (f32x3) weight planes: 0 = not taken (the igemm runs), 1 = 8x8, 2 = 8x16 patches. */
int ssd_conv2d_wgrad_plan(const ssd_conv_geom* g, int bf16, int* plan);
int ssd_conv3x3_bf16_plan(int N, int H, int W, int K, int n_out, int* plan);
int ssd_conv3x3_halo_shape(const ssd_conv_geom* g, int direction, int planes);
/* Tuning aids (process-global, not thread-safe, results unchanged): force the igemm tile
 * (0 = 256x64, 1 = 128x128, 2 = 128x64, 3 = 64x64) / LDS stage count (1|2), and the wgrad tile edge
 * (64|128) / stage count / split-K target in blocks per CU.  -1 = automatic. */
/* Same convolutions with an optional scratch buffer: launches whose 64x64-tile grid would leave most of the chip idle
 * while each block walks a long K loop (the 19x19 and smaller maps: c_7 ... c_11, seq8 ... seq11) are split along K
 * into partial tiles in the workspace and finished (bias / accumulate / ReLU / mask) by a fixed-order reduction.
 * workspace may be NULL or smaller than ssd_conv2d_igemm_workspace(g, direction) asks: the launch is then not split. */
size_t ssd_conv2d_igemm_workspace(const ssd_conv_geom* g, int direction /* 0 forward, 1 dgrad */);
int ssd_conv2d_fwd_ws(const float* x, const float* w_ohwi, const float* bias, float* y, int ldy, const ssd_conv_geom* g,
                      int relu, void* workspace, size_t workspace_bytes, void* stream);
int ssd_conv2d_dgrad_ws(const float* dy, int ldy, const float* w_ihwo, int Co_pad, float* dx, const float* relu_mask,
                        int accumulate, const ssd_conv_geom* g, void* workspace, size_t workspace_bytes, void* stream);
int ssd_tune_set_igemm_splitk(int k);       /* -1 automatic, 1 never split, k > 1 force k slices */
/* ---- Winograd F(mo x mo, 3x3), mo = 2 or 4, for the 3x3 / stride 1 / pad 1 layers: (mo+2)^2 multiplies per mo x mo output tile
 * instead of 9 mo^2 (2.25x / 4x fewer).  Results differ from the direct sum at the 1e-6 (mo = 2) / 1e-5 (mo = 4) level of the
 * output scale.  ssd_wino_weights transforms the OIHW filter once per update: U_fwd [P][Co][Ci] for the forward, U_bwd
 * [P][Ci][Co_pad] (transposed, rotated filter) for dgrad, P = (mo+2)^2; either may be NULL.  The convolutions take the
 * transformed filter, a workspace of ssd_conv3x3_wino_workspace(g, direction, mo) bytes, and fuse the direct kernels' epilogues. */
int ssd_wino_weights(const float* w_oihw, float* U_fwd, float* U_bwd, int Co, int Ci, int Co_pad, int mo, void* stream);
size_t ssd_conv3x3_wino_workspace(const ssd_conv_geom* g, int direction /* 0 forward, 1 dgrad */, int mo);
int ssd_conv3x3_wino_fwd(const float* x, const float* U_fwd, const float* bias, float* y, int ldy, const ssd_conv_geom* g, int relu,
                         int mo, void* workspace, size_t workspace_bytes, void* stream);
int ssd_conv3x3_wino_dgrad(const float* dy, int ldy, const float* U_bwd, int Co_pad, float* dx, const float* relu_mask,
                           int accumulate, const ssd_conv_geom* g, int mo, void* workspace, size_t workspace_bytes, void* stream);
/* conv3x3 -> ReLU -> MaxPool2d(2, 2, ceil_mode) in one pass (Model.py:135-137 via the VGG layer list: conv1_2, conv2_2, conv3_3 and
 * their pools): F(4x4,3x3) whose output transform reduces each 4x4 tile to its four pool windows, so the full-resolution
 * activation -- read by nothing but the pool -- is never written.  y_pooled (N,Ho,Wo,Co), Ho = H/2 (ceil_mode: (H+1)/2); argmax
 * (may be NULL) in ssd_maxpool_fwd's encoding, for ssd_maxpool_bwd / ssd_maxpool_bwd_gated.  Co % 4 == 0; workspace as
 * ssd_conv3x3_wino_workspace(g, 0, 4).  Equal, bit for bit, to ssd_conv3x3_wino_fwd(relu = 1, mo = 4) followed by ssd_maxpool_fwd.
 * planes_keep (may be NULL): see ssd_conv3x3_wino_fwd_keep. */
int ssd_conv3x3_wino_fwd_pool(const float* x, const float* U_fwd, const float* bias, float* y_pooled, uint8_t* argmax,
                              const ssd_conv_geom* g, int ceil_mode, float* planes_keep, void* workspace, size_t workspace_bytes,
                              void* stream);
/* F(4x4,3x3) forward that leaves the transformed input B^T d B in planes_keep -- 36 x tiles x Ci floats, tiles = N ceil(H/4) ceil(W/4),
 * layout [plane][tile][channel] -- for ssd_conv3x3_wino_wgrad_planes, which then skips transforming x a second time in the backward
 * pass (the planes are 2.25x the activation; 288 GB of HBM pay for that).  Otherwise ssd_conv3x3_wino_fwd with mo = 4. */
int ssd_conv3x3_wino_fwd_keep(const float* x, const float* U_fwd, const float* bias, float* y, int ldy, const ssd_conv_geom* g, int relu,
                              float* planes_keep, void* workspace, size_t workspace_bytes, void* stream);
/* Winograd weight gradient: dg = G^T [ sum over tiles (A dy A^T) (x) (B^T d B) ] G -- transposed transforms of dy and x, sixteen
 * batched (split-K) f32-MFMA GEMMs over the tile dimension, inverse transform to OIHW; dbias (may be NULL) by column sums. */
size_t ssd_conv3x3_wino_wgrad_workspace(const ssd_conv_geom* g, int ldy, int mo);
int ssd_conv3x3_wino_wgrad(const float* x, const float* dy, int ldy, float* dw_oihw, float* dbias, const ssd_conv_geom* g, int mo,
                           void* workspace, size_t workspace_bytes, void* stream);
/* The same with the x planes a ..._fwd_keep / ..._fwd_pool call kept (F(4x4) only); workspace as ssd_conv3x3_wino_wgrad_workspace(g, ldy, 4).
 * dgrad_planes_out (may be NULL; 36 x tiles x ldy floats): the pass over dy also writes B^T dy B, the input planes of this layer's
 * data gradient, which ssd_conv3x3_wino_dgrad_planes (Co_pad = ldy) then takes instead of transforming dy again. */
/* Every filter transform / re-layout of a training step in one launch.  A job: kind 0 = Winograd F(4x4,3x3) filters (out_fwd [36][co][ci],
 * out_bwd [36][ci][co_pad]: the transposed, rotated filter of the data gradient), kind 1 = the direct kernels' copies (out_fwd OHWI
 * [co_pad][taps][ci], out_bwd IHWO [ci][taps][co_pad]), kind 2 = conv1_1's rows for the im2col GEMM (out_fwd [co][32]).  The OIHW source
 * may come in two pieces (rows 0..co0-1 from w0, the rest from w1: a head's loc and conf filters); out_bwd may be NULL.  The caller
 * uploads the job array and the exclusive prefix sum of ssd_weight_job_blocks(job) (block_start, njobs entries) to the device once. */
typedef struct ssd_weight_job {
    const float* w0; const float* w1;
    float* out_fwd; float* out_bwd;
    int co0, co, ci, taps, co_pad, kind, pad0, pad1;
} ssd_weight_job;
int ssd_weight_job_blocks(const ssd_weight_job* job);
int ssd_weights_prepare(const ssd_weight_job* jobs_device, const int* block_start_device, int njobs, int total_blocks, void* stream);
/* The F(4x4) weight gradient on kept planes as two calls, so that the caller can put the second on another stream: nothing in the
 * backward pass waits for dw, while the data gradient waits for dgrad_planes_out.  (1) ssd_wino4_dy_transform: one pass over dy ->
 * wgrad_planes (36 x tiles x ldy: A dy A^T), optionally dgrad_planes_out (36 x tiles x ldy: B^T dy B, for ssd_conv3x3_wino_dgrad_planes)
 * and bias_partial (ssd_wino4_bias_partial_floats(g, ldy) floats: per-block column sums of dy; needs ldy <= 1024).
 * (2) ssd_wino4_wgrad_gemm: the 36 split-K TN GEMMs wgrad_planes^T x x_planes, inverse transform to OIHW, and dbias from bias_partial;
 * workspace ssd_wino4_wgrad_gemm_workspace(g, ldy) bytes.  Together they equal ssd_conv3x3_wino_wgrad_planes bit for bit. */
size_t ssd_wino4_bias_partial_floats(const ssd_conv_geom* g, int ldy);
int ssd_wino4_dy_transform(const float* dy, int ldy, const ssd_conv_geom* g, float* wgrad_planes, float* dgrad_planes_out,
                           float* bias_partial, void* stream);
size_t ssd_wino4_wgrad_gemm_workspace(const ssd_conv_geom* g, int ldy);
int ssd_wino4_wgrad_gemm(const float* wgrad_planes, const float* x_planes, int ldy, const float* bias_partial, float* dw_oihw, float* dbias,
                         const ssd_conv_geom* g, void* workspace, size_t workspace_bytes, void* stream);
/* The same two passes when dy is the gradient of the 2x2 / stride-2 / no-pad max pool that is the only reader of this layer's ReLU output
 * (ssd_conv3x3_wino_fwd_pool): dy is never written to memory.  The pass takes the pooled gradient dpool (N x Hp x Wp x Co), the argmax
 * codes and the pooled forward output of that pool (its ReLU gate) and forms dy(h, w) on the fly -- what ssd_maxpool_bwd_gated would
 * have scattered (reference: autograd of MaxPool2d(ReLU(conv)), Model.py:135-137).  ldy must equal Co; Hp = H/2 or (H+1)/2. */
int ssd_wino4_dy_transform_pooled(const float* dpool, const unsigned char* argmax, const float* y_pooled, int Hp, int Wp, int ldy,
                                  const ssd_conv_geom* g, float* wgrad_planes, float* dgrad_planes_out, float* bias_partial, void* stream);
int ssd_conv3x3_wino_wgrad_planes_pooled(const float* planes, const float* dpool, const unsigned char* argmax, const float* y_pooled,
                                         int Hp, int Wp, int ldy, float* dw_oihw, float* dbias, const ssd_conv_geom* g,
                                         float* dgrad_planes_out, void* workspace, size_t workspace_bytes, void* stream);
/* ReLU masks as bits.  The forward's input transform can leave, per (tile, channel quad), one 64-bit word -- bit (a*4+b)*4+e set iff
 * x[4 th + a][4 tw + b][4 c4 + e] > 0 -- in relu_bits_out (tiles x Ci/4 words; may be NULL): the ReLU mask of the layer's INPUT on the tile
 * grid its data gradient is written on (autograd's ReLU backward, Model.py:136-141).  ssd_conv3x3_wino_dgrad_planes_bits applies it in
 * place of ssd_conv3x3_wino_dgrad_planes's float relu_mask, reading 1/32 of the bytes; results are identical. */
int ssd_conv3x3_wino_fwd_keep_bits(const float* x, const float* U_fwd, const float* bias, float* y, int ldy, const ssd_conv_geom* g, int relu,
                                   float* planes_keep, uint64_t* relu_bits_out, void* workspace, size_t workspace_bytes, void* stream);
int ssd_conv3x3_wino_fwd_pool_bits(const float* x, const float* U_fwd, const float* bias, float* y_pooled, uint8_t* argmax,
                                   const ssd_conv_geom* g, int ceil_mode, float* planes_keep, uint64_t* relu_bits_out, void* workspace,
                                   size_t workspace_bytes, void* stream);
int ssd_conv3x3_wino_dgrad_bits(const float* dy, int ldy, const float* U_bwd, int Co_pad, float* dx, const uint64_t* relu_bits, int accumulate,
                                const ssd_conv_geom* g, void* workspace, size_t workspace_bytes, void* stream);
int ssd_conv3x3_wino_dgrad_planes_bits(const float* dy_planes, const float* U_bwd, int Co_pad, float* dx, const uint64_t* relu_bits,
                                       int accumulate, const ssd_conv_geom* g, void* workspace, size_t workspace_bytes, void* stream);
int ssd_conv3x3_wino_wgrad_planes(const float* planes, const float* dy, int ldy, float* dw_oihw, float* dbias, const ssd_conv_geom* g,
                                  float* dgrad_planes_out, void* workspace, size_t workspace_bytes, void* stream);
int ssd_conv3x3_wino_dgrad_planes(const float* dy_planes, const float* U_bwd, int Co_pad, float* dx, const float* relu_mask,
                                  int accumulate, const ssd_conv_geom* g, void* workspace, size_t workspace_bytes, void* stream);
/* conv1_1 written as the next layer's Winograd input (round 4 EXPERIMENT: ssd_conv1_first_wino_fwd returns SSD_ERR_BAD_SHAPE unless built
 * with SSD_EXPERIMENTAL=1 -- bit-identical but measured slower than the two kernels it replaces; Model.py:135 features[0:4]:
 * Conv2d(3,64) -> ReLU -> Conv2d(64,64)).  In
 * training nothing but conv1_2 reads conv1_1's activation, so ssd_conv1_first_wino_fwd leaves it as the F(4x4) input planes
 * (36 x N*ceil(H/4)*ceil(W/4) x 64 f32) + the ReLU bit words of ssd_conv3x3_wino_fwd_keep_bits, bit-identical to ssd_conv1_first_fwd followed
 * by that layer's input transform, and the 64-channel activation (737 MB at batch 32) is neither written nor read.
 * ssd_conv3x3_wino_fwd_from_planes is the forward of a layer whose planes are given: plane GEMMs + output transform (+ the fused 2x2 pool
 * when y_pooled is not NULL; then y may be NULL). */
int ssd_conv1_first_wino_fwd(const float* x_nchw, const float* w_rows, const float* bias, float* planes, uint64_t* relu_bits, int N, int H, int W,
                             void* stream);
int ssd_conv3x3_wino_fwd_from_planes(const float* planes, const float* U_fwd, const float* bias, float* y, int ldy, float* y_pooled, uint8_t* argmax,
                                     const ssd_conv_geom* g, int relu, int ceil_mode, void* workspace, size_t workspace_bytes, void* stream);
/* Data gradient in the ADJOINT Winograd form (round 4; autograd of nn.Conv2d, reference Model.py:135-143 / train_function.py:94).
 * The forward y = A^T[(G g G^T) (.) (B^T d B)]A is linear in d; transposed, dx = overlap-add over the tiles of the 6x6 patches
 * B[(G g G^T) (.) (A dy A^T)]B^T: the data gradient multiplies the SAME planes A dy A^T (ssd_wino4_dy_transform's wgrad_planes) the
 * weight gradient multiplies, so the second plane set B^T dy B (dgrad_planes_out) is neither written nor read, against the forward
 * filter transform laid out [36][Ci][Co_pad] (ssd_wino_weights_adj; weight jobs: pad0 bit 2; f32 or limb planes by
 * ssd_wino_uses_x3(4, Co_pad)).  (1) ssd_conv3x3_wino_dgrad_adj_gemm: md_planes (ssd_wino4_adj_planes_floats(g) floats:
 * 36 x tiles x pad4(Ci)) = y_planes x U_adj, ldy % 32 == 0.  (2a) ssd_wino4_adj_output: dx (N,H,W,Ci) [+=] the overlap-added patches,
 * ReLU-masked by relu_bits (as left by ssd_conv3x3_wino_fwd_keep_bits) or by the f32 tensor relu_mask (either may be NULL); or
 * (2b) ssd_wino4_adj_output_to_planes: the same block of dx is not stored but taken, masked, as the dy of the layer BELOW (g_below:
 * same map, Co = g->Ci) and leaves that layer's planes A dy A^T (36 x tiles x g->Ci) and bias partial sums
 * (ssd_wino4_bias_partial_floats(g_below, g->Ci); may be NULL): between two chained 3x3 layers the gradient tensor never reaches memory.
 * 3x3 / stride 1 / pad 1 / dilation 1 only. */
int ssd_wino_weights_adj(const float* w_oihw, float* U_adj, int Co, int Ci, int Co_pad, void* stream);
size_t ssd_wino4_adj_planes_floats(const ssd_conv_geom* g);
int ssd_conv3x3_wino_dgrad_adj_gemm(const float* y_planes, int ldy, const float* U_adj, float* md_planes, const ssd_conv_geom* g, void* stream);
int ssd_wino4_adj_output(const float* md_planes, float* dx, const float* relu_mask, const uint64_t* relu_bits, int accumulate,
                         const ssd_conv_geom* g, void* stream);
int ssd_wino4_adj_output_to_planes(const float* md_planes, const float* relu_mask, const uint64_t* relu_bits, const ssd_conv_geom* g,
                                   const ssd_conv_geom* g_below, float* y_planes, float* bias_partial, void* stream);
/* Forward / dgrad of the F(4x4,3x3) entry points: 36 plane GEMMs + output transform in ONE kernel (accumulators of all planes in
 * registers, the M planes never reach memory) where the reduction length is a multiple of 64.  -1 (default): where it is the faster
 * form; 0: never (batched GEMM + output transform kernels); 1: wherever the geometry allows. */
int ssd_tune_set_wino_bias_tail(int on);   /* 1 (default): the bias gradient's final column sums run as extra blocks of the weight gradient's finish kernel; 0: own launch */
int ssd_tune_set_wino_xform_blocks(int blocks);   /* grid cap of the Winograd transform kernels (default 8192; 64 .. 65535) */
int ssd_tune_set_wino_fused(int mode);
/* Experiment (round 4, csrc/gemm_x3v2.hip; SSD_EXPERIMENTAL builds only -- otherwise SSD_ERR_BAD_SHAPE; not on the step's path): the same plane GEMMs with BOTH operands given as limb planes of
 * ssd_gemm_x3_split_weights (a3: rows = M, w3: rows = n_rows), 256 x 256 tiles, LDS-DMA on both sides, two wave groups in ping-pong.
 * dither = 1: a3's rows carry the sign s(m) of csrc/gemm_x3.hip and the result is multiplied by it again. */
int ssd_gemm_planes_x3v2(const void* a3, const void* w3, float* out, int M, int K, int N, int n_rows, int nbatch, int dither, void* stream);
int ssd_tune_set_x3_big(int mode);         /* limb plane GEMMs: 0 (default) = always the 128 x 128 kernel; SSD_EXPERIMENTAL builds only: 1 = launches with N >= 256 and M >= 2048 on the 256 x 256 ping-pong kernel (csrc/gemm_x3v2.hip), 2 = every launch it takes */
int ssd_tune_set_x3_mfma(int rows);        /* limb plane GEMMs (csrc/gemm_x3.hip): 32 (default) = v_mfma_f32_32x32x16_bf16; SSD_EXPERIMENTAL builds only: 16 = v_mfma_f32_16x16x32_bf16, two limb products per instruction */
/* The plane GEMMs of the layers that do not take the one-kernel form: persistent 128 x 128 LDS-DMA kernel (gemm_nt.hip) instead of the
 * generic 64 x 64 implicit-GEMM kernel.  1: wherever K % 32 == 0 and K >= 64; -1 (default) / 0: never -- measured no faster (both kernels
 * sit at the device's sustained f32 MFMA rate); kept, tested bit-identical, as the evidence for that statement. */
int ssd_tune_set_gemm_nt(int mode);
/* f32 plane GEMMs on the bf16 MFMA from three exact bf16 limbs per operand (csrc/gemm_x3.hip; the Winograd-domain products of the
 * 3x3 layers, Model.py:135-156): out[b][m][n] = sum_k a[b][m][k] * w[b][n][k].  The filter planes are split once
 * (ssd_gemm_x3_split_weights: w [nbatch][rows][K] f32 -> w3, ssd_gemm_x3_weights_bytes(rows, K, nbatch) bytes); K % 16 == 0, n_rows >= N.
 * ssd_gemm_planes_f32: the same product on the f32 MFMA (K % 32 == 0), the kernel the x3 form replaces -- both are public for the
 * parity test and tools/gemm_x3_bench.py. */
/* ssd_wino_uses_x3(mo, K): 1 if the F(4x4) plane GEMMs of reduction length K run the three-limb form -- the transformed filter of such
 * a layer (U_fwd: K = Ci; U_bwd: K = Co_pad) is then NOT [36][rows][K] f32 but [36][K/16][3][pad128(rows)][16] bf16 limbs
 * (ssd_gemm_x3_weights_bytes(rows, K, 36) bytes, zero-initialised by the caller: padding rows are never written), both from
 * ssd_wino_weights and from a kind-0 weight job with bit 0 (out_fwd) / bit 1 (out_bwd) of pad0 set.  ssd_tune_set_wino_x3(0 | 1 | -1):
 * off / on / the default (environment SSD_WINO_X3, on unless "0"); filters transformed under one setting must not be used under another. */
int ssd_wino_uses_x3(int mo, int K);
int ssd_tune_set_wino_x3(int on);
size_t ssd_gemm_x3_weights_bytes(int rows, int K, int nbatch);
int ssd_gemm_x3_split_weights(const float* w, void* w3, int rows, int K, int nbatch, void* stream);
int ssd_gemm_planes_x3(const float* a, const void* w3, float* out, int M, int K, int N, int n_rows, int nbatch, void* stream);
/* 1x1 / stride-1 convolutions with long reductions (fc7, seq8.0: Model.py:150-156) on the same limb kernels.  Filters as limb planes:
 * forward w3 = limbs of w [Co][Ci] (ssd_gemm_x3_split_weights(w, w3, Co, Ci, 1), or a kind-4 job of ssd_weights_prepare: out_fwd rows Co,
 * K = Ci; out_bwd rows Ci, K = co_pad = limbs of w^T); Ci % 32 == 0 forward, ldy = Co_pad % 32 == 0 for the data gradient (the reduction
 * runs over all ldy columns of dy: padding columns must be zero).  Epilogues as ssd_conv2d_fwd / ssd_conv2d_dgrad. */
int ssd_conv1x1_fwd_x3(const float* x, const void* w3, const float* bias, float* y, int ldy, const ssd_conv_geom* g, int relu, void* stream);
int ssd_conv1x1_dgrad_x3(const float* dy, int ldy, const void* w3t, float* dx, const float* relu_mask, int accumulate, const ssd_conv_geom* g,
                         void* stream);
size_t ssd_conv1x1_wgrad_x3_workspace(const ssd_conv_geom* g, int ldy);
int ssd_conv1x1_wgrad_x3(const float* x, const float* dy, int ldy, float* dw, float* dbias, const ssd_conv_geom* g, void* workspace,
                         size_t workspace_bytes, void* stream);
int ssd_gemm_planes_f32(const float* a, const float* w, float* out, int M, int K, int N, int n_rows, int nbatch, void* stream);
int ssd_has_experimental(void);           /* 1 if built with SSD_EXPERIMENTAL: gemm_nt.hip and wino4_full_kernel (both off by default, forced by ssd_tune_set_gemm_nt(1) / ssd_tune_set_wino_full(1)) are present */
/* The whole convolution (input transform too) in one kernel where the reduction length is 64 (128 when forced): -1 automatic, 0 never, 1 force.
 * ssd_conv3x3_wino_uses_full tells the caller whether a geometry's forward (0) / data gradient from dy (1) takes that kernel -- it then
 * needs no dgrad planes from ssd_wino4_dy_transform. */
int ssd_tune_set_wino_full(int mode);
int ssd_conv3x3_wino_uses_full(const ssd_conv_geom* g, int direction);
int ssd_tune_set_wino_fused_stagger(int cycles);   /* first-round start delay step between CUs (shader cycles); -1 / 0 (default): none */
int ssd_tune_set_wino_fused_stamps(uint64_t* device_buffer);   /* diagnostic: in-kernel phase stamps of the fused kernel; NULL = off */
int ssd_tune_set_wino_wgrad_tn(int on);   /* 1 (default): F(4x4) weight gradient on untransposed planes + TN GEMM; 0: transposed planes */
/* Measurement aid: arm / read back per-launch timings (library-owned HIP events) of the batched Winograd GEMM kernel.
 * collect() returns the number of (milliseconds, executed FLOPs) pairs written; the caller synchronises the stream first. */
int ssd_prof_gemm_begin(void);
int ssd_prof_gemm_collect_kinds(float* ms_out, double* flops_out, int* kinds_out, int max);   /* kind 0: batched plane GEMMs, 1: fused GEMM + output transform */
int ssd_prof_gemm_collect(float* ms_out, double* flops_out, int max);
int ssd_tune_set_igemm(int tile, int nbuf);
int ssd_tune_set_igemm_stamps(uint64_t* device_buffer);   /* diagnostic: per-block shader-clock stamps (see conv_igemm.hip) */
int ssd_tune_set_dgrad_parity(int on);   /* 1 (default): data gradients of stride-2 convolutions with their rows grouped by pixel parity (only the taps that reach a class are multiplied); 0: plain kernel */
int ssd_tune_set_batched_units(int on);   /* 1 (default): the blocks of one (plane, part of the row tiles) of a batched plane GEMM share one XCD; 0: 3-D grid */
int ssd_tune_set_igemm_lds_pad(int bytes);   /* extra dynamic LDS per block: caps resident blocks per CU (experiments) */
int ssd_tune_set_wgrad(int bt, int nbuf, int blocks_per_cu);
int ssd_tune_set_wgrad_patch(int shape);     /* f32 fused 3x3 kernel: -1 least padding, 0 = 4x8 pixel patches, 1 = 1x38, 2 = 2x19 */

/* conv1_1 (Model.py:136 features[0]: Conv2d(3,64,3,padding=1)+ReLU, Ci = 3): im2col of the caller's
 * NCHW image batch (Dataset.py:39 layout) into [N*H*W][32] rows (k = (r*3+s)*3 + c, columns 27..31
 * zero); forward / wgrad are then the 1x1 cases of ssd_conv2d_fwd / ssd_conv2d_wgrad with Ci = 32. */
int ssd_im2col_first(const float* x_nchw, float* out, int N, int H, int W, void* stream);
/* conv1_1 + ReLU in one kernel (Model.py:135, features[0:2]): x (N,3,H,W) NCHW -> y (N,H,W,64) NHWC = relu(conv3x3 pad 1 + bias).
 * w_rows: [64][32] filter rows in ssd_im2col_first's column order (k = (r*3+s)*3 + c, columns 27..31 zero).  col_out (may be NULL):
 * the same pass also writes the (N,H,W,32) rows ssd_im2col_first would, for the weight gradient (ssd_conv2d_wgrad on them). */
int ssd_conv1_first_fwd(const float* x_nchw, const float* w_rows, const float* bias, float* y_nhwc, float* col_out, int N, int H, int W,
                        int relu, void* stream);
/* Weight and bias gradient of conv1_1 from the NCHW input itself (autograd of Model.py:135 features[0]): dw_rows [64][32] in the column
 * order above (columns 27..31 zero; ops.first_weight_grad turns them into OIHW), dbias [64] (may be NULL) = sum of dy over the pixels.
 * dy (N,H,W,64) NHWC dense.  Workspace ssd_conv1_first_wgrad_workspace bytes (partial sums of the persistent workgroups, added in order). */
size_t ssd_conv1_first_wgrad_workspace(int N, int H, int W);
int ssd_conv1_first_wgrad(const float* x_nchw, const float* dy_nhwc, float* dw_rows, float* dbias, int N, int H, int W, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- SSD_resnet34 (Model.py:12-126, BASELINE configs[4]) eval-mode forward pieces ----
 * Stem Conv2d(3,64,7,stride 2,pad 3) (Model.py:26 seq1[0]): general 3-channel NCHW im2col into [N*Ho*Wo][Kpad]
 * rows (k = (r*S+s)*3 + c, zero from R*S*3 to Kpad; Kpad % 32 == 0 for the 1x1 case of ssd_conv2d_fwd). */
int ssd_im2col_nchw3(const float* x_nchw, float* out, int N, int H, int W, int R, int S, int stride, int pad,
                     int Ho, int Wo, int Kpad, void* stream);
/* BasicBlock tail `relu(bn2(conv2(o)) + identity)` (torchvision layer list sliced at Model.py:27-30): the
 * convolution (BatchNorm folded into w / bias by the host) is ADDED to y_inout, which holds the identity /
 * downsample branch on entry, then ReLU'd in place. */
int ssd_conv2d_fwd_accum(const float* x, const float* w_ohwi, const float* bias, float* y_inout, int ldy,
                         const ssd_conv_geom* g, int relu, void* stream);
int ssd_conv2d_fwd_accum_bf16(const float* x, const float* w_ohwi, const float* bias, float* y_inout, int ldy,
                              const ssd_conv_geom* g, int relu, void* stream);
/* eval-mode BatchNorm2d after a ReLU (Model.py:56-62 Conv -> ReLU -> BN -> Dropout2d): y = x*scale[c] + shift[c]
 * over [M][C] NHWC rows, C % 4 == 0, optional ReLU; x may alias y. */
int ssd_channel_affine(const float* x, const float* scale, const float* shift, float* y, size_t M, int C, int relu,
                       void* stream);

/* ---- max pooling (Model.py:137,142 nn.MaxPool2d incl. ceil_mode; features[4,9,23]) ----
 * argmax: uint8 window-relative index (r*k+s) of the first maximum, for backward.  A NaN replaces the running maximum (torch's rule), so
 * the last NaN of a window wins.  What these entries, the L2 norm and the heads refuse: REFUSALS above, next to the bf16 forms. */
int ssd_maxpool_fwd(const float* x, float* y, uint8_t* argmax, int N, int H, int W, int C,
                    int k, int stride, int pad, int Ho, int Wo, void* stream);
/* dx (+)= routed dy; if relu_mask != NULL dx = relu_mask > 0 ? dx : 0. */
int ssd_maxpool_bwd(const float* dy, const uint8_t* argmax, float* dx, const float* relu_mask, int accumulate,
                    int N, int H, int W, int C, int k, int stride, int pad, int Ho, int Wo, void* stream);
/* Same gradient for a pool whose input is a ReLU output and has no other consumer: dx = relu_mask(x) * scatter(dy) computed
 * as scatter(dy gated by y > 0), y = the pooled output (an arg-max input equals its window's output) -- reads y instead of
 * the 4x larger x. */
int ssd_maxpool_bwd_gated(const float* dy, const uint8_t* argmax, const float* y, float* dx, int N, int H, int W, int C,
                          int k, int stride, int pad, int Ho, int Wo, void* stream);

/* ---- conv4_3 L2 normalisation (Model.py:206-209): y = x / sqrt(sum_c x^2) * gamma_c, no epsilon */
int ssd_l2norm_fwd(const float* x, const float* gamma, float* y, int M, int C, void* stream);
size_t ssd_l2norm_bwd_workspace(int M, int C);
int ssd_l2norm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma,
                   int M, int C, void* workspace, size_t workspace_bytes, void* stream);

/* ---- head output <-> (bs,P,4)/(bs,P,n_classes) (Model.py:212-235 permute+view+cat) ------------
 * n_classes = conf width C (foreground classes + background), 21 for VOC.
 * packed[m][0:4A] = loc channels, packed[m][4A:(4+C)A] = conf channels of pixel m=(n,h,w);
 * prior index = prior_off + (h*W+w)*A + a. */
int ssd_heads_scatter(const float* packed, int ld, float* loc, float* conf, int N, int HW, int A,
                      int prior_off, int P, int n_classes, void* stream);
int ssd_heads_gather(const float* dloc, const float* dconf, float* packed, int ld, int N, int HW, int A,
                     int prior_off, int P, int n_classes, void* stream);

/* ---- MultiBox loss (Losses.py:119-199 ssd + ssd1_; Util.py:57-63,98-102,252-301) -------
 * n_classes = conf width C, 2..256 (foreground classes + background; background = C-1 is the last column).
 * gt_boxes (n_gt,4) xyxy f32, gt_classes (n_gt) f32 values 0..C-2 (other values: unspecified losses, but every
 * kernel clamps the label into the row -- no access outside the tensors), img_start (bs+1) int32
 * prefix offsets into them (every image needs >= 1 box: checked by the caller on the host,
 * the reference raises there).  priors_cxcywh/priors_xyxy (P,4).
 * Outputs: losses[0]=loc_loss, losses[1]=conf_loss, losses[2]=n_pos (as float);
 *          obj (bs,P) int32 global GT index; cls (bs,P) int32 (bg_class = n_classes-1);
 *          dloc/dconf = d(loc_loss+conf_loss)/d(loc|conf) (may both be NULL: forward only).
 * norm_mode 0: reference normalisation (divide by batch n_pos).
 * norm_mode 1: un-normalised sums (loc: sum|d|/4, conf: sum CE) and gradients of those,
 *              for data-parallel runs that divide by the global n_pos after the all-reduce.
 * Three kernel launches (per-prior matching + cross entropy, wide; per-image forced matches + hard-negative selection; losses +
 * gradients, wide); ssd_tune_set_loss_form(0) selects the four-launch form of rounds 1-3 (cross-check).  C <= 64 stages conf rows
 * in LDS; 64 < C <= 256 runs the wide-row forms of the first and last kernel (a wave across a row's classes, nothing staged per class). */
int ssd_tune_set_loss_form(int three_launch);
size_t ssd_multibox_loss_workspace(int bs, int P, int n_gt);
int ssd_multibox_loss(const float* loc, const float* conf, const float* gt_boxes, const float* gt_classes,
                      const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh,
                      const float* priors_xyxy, int P, int n_classes, float iou_threshold, int neg_pos_ratio,
                      int norm_mode, float* losses, int32_t* obj, int32_t* cls, float* dloc, float* dconf,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- MultiBox loss with ignore regions (VOC `difficult` objects, COCO crowd regions) ----------
 * ssd_multibox_loss's arguments, meaning and status codes, plus:
 *   ign_boxes (n_ign,4) xyxy f32, fractional like gt_boxes; may be NULL when n_ign == 0.
 *   ign_start (bs+1) int32 ON THE DEVICE: prefix offsets into ign_boxes (data, as img_start is: a captured call replays any
 *             split of the boxes over the images, an image may have none).  n_ign = total number of ignore boxes, >= 0.
 *   ignore_threshold, overlap_mode: a prior that is NOT positive is ignored when some ignore box of its image overlaps it by
 *             >= ignore_threshold.  overlap_mode 0: IoU (the matching's f32 op sequence); 1: intersection / the prior's own
 *             unclipped area (the crowd rule of the COCO protocol with the prior in the detection's place).  A NaN overlap
 *             ignores nothing.
 *   ign (bs,P) uint8 output: 1 for an ignored prior.
 * Matching takes no notice of ignore boxes: a positive prior (threshold or forced match) stays positive.  An ignored prior is
 * treated in the hard-negative mining as the positives are (mining value 0; ranking, quota min(ratio * n_pos, P) and the
 * lower-index-first tie rule are unchanged) and receives no gradient: its dconf and dloc rows are exactly zero, also when the
 * quota reaches into the zero values.  With no ignore box in any image every output equals ssd_multibox_loss's bit for bit.
 * Always the three-launch form: ssd_tune_set_loss_form does not reach this entry (the four-launch cross-check form has no
 * ignore path).  The workspace is ssd_multibox_loss's.
 * Errors: SSD_ERR_NULL (a null pointer; ign_boxes null with n_ign > 0), SSD_ERR_BAD_SHAPE (the shape rules above, n_ign < 0,
 * overlap_mode not 0 / 1), SSD_ERR_ALIGN (ign_boxes not 16-byte aligned, besides the rules above), SSD_ERR_WORKSPACE. */
size_t ssd_multibox_loss_ignore_workspace(int bs, int P, int n_gt, int n_ign);
int ssd_multibox_loss_ignore(const float* loc, const float* conf, const float* gt_boxes, const float* gt_classes,
                             const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh,
                             const float* priors_xyxy, int P, int n_classes, float iou_threshold, int neg_pos_ratio,
                             int norm_mode, const float* ign_boxes, const int32_t* ign_start, int n_ign,
                             float ignore_threshold, int overlap_mode, float* losses, int32_t* obj, int32_t* cls,
                             uint8_t* ign, float* dloc, float* dconf, void* workspace, size_t workspace_bytes, void* stream);

/* ---- MultiBox loss with a choice of localisation term (IoU, GIoU, DIoU, CIoU) ----------
 * ssd_multibox_loss_ignore's arguments, meaning and status codes, plus int loc_mode: 0 = L1 (the reference's term), 1 = IoU,
 * 2 = GIoU, 3 = DIoU, 4 = CIoU.  ign_start == NULL means "no ignore regions": ign, ign_boxes, n_ign, ignore_threshold and
 * overlap_mode are then not looked at (ign and ign_boxes may be NULL) and nothing is written to ign.
 * For a positive prior (pcx, pcy, pw, ph) with offsets l and matched box g = (gx1, gy1, gx2, gy2), T = log(1000 / 16), eps = 1e-7:
 *   cx = l0 pw / 10 + pcx, cy = l1 ph / 10 + pcy, w = exp(clamp(l2 / 5, -T, T)) pw, h = exp(clamp(l3 / 5, -T, T)) ph,
 *   (x1, y1, x2, y2) = (cx - w/2, cy - h/2, cx + w/2, cy + h/2), gw = gx2 - gx1, gh = gy2 - gy1,
 *   inter = max(min(x2, gx2) - max(x1, gx1), 0) max(min(y2, gy2) - max(y1, gy1), 0), union = w h + gw gh - inter,
 *   iou = inter / (union + eps), cw = max(x2, gx2) - min(x1, gx1), ch = max(y2, gy2) - min(y1, gy1),
 *   1: L = 1 - iou                                  2: L = 1 - iou + (cw ch - union) / (cw ch + eps)
 *   3: L = 1 - iou + rho2 / (cw^2 + ch^2 + eps), rho2 = squared distance of the two centres
 *   4: L = (3) + alpha v, v = 4 / pi^2 (atan(gw / gh) - atan(w / h))^2, alpha = v / (1 - iou + v + eps), a constant of the gradient
 *      (needs gh > 0; modes 1 .. 3 take boxes without area).
 * losses[0] = sum of L over the positives / n_pos (norm_mode 0) or the sum itself (norm_mode 1); dloc is the gradient of that value,
 * exactly zero at non-positive priors and at a clamped coordinate.  Mode 1 has no gradient where the boxes do not overlap.
 * Matching, n_pos, the hard-negative quota and selection, ignore regions, losses[1], losses[2] and dconf do not depend on loc_mode.
 * loc_mode 0 launches the very kernels of ssd_multibox_loss (ign_start NULL) or ssd_multibox_loss_ignore; always the three-launch
 * form.  The workspace is ssd_multibox_loss's.
 * Errors: as ssd_multibox_loss_ignore (its ignore rules only with ign_start given); loc_mode outside 0 .. 4 is SSD_ERR_BAD_SHAPE. */
size_t ssd_multibox_loss_box_workspace(int bs, int P, int n_gt, int n_ign);
int ssd_multibox_loss_box(const float* loc, const float* conf, const float* gt_boxes, const float* gt_classes,
                          const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh, const float* priors_xyxy,
                          int P, int n_classes, float iou_threshold, int neg_pos_ratio, int norm_mode, const float* ign_boxes,
                          const int32_t* ign_start, int n_ign, float ignore_threshold, int overlap_mode, int loc_mode,
                          float* losses, int32_t* obj, int32_t* cls, uint8_t* ign, float* dloc, float* dconf, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- MultiBox loss with a choice of classification term (sigmoid focal loss, Lin et al. 2017) ----------
 * ssd_multibox_loss_box's arguments, meaning and status codes, plus int conf_mode (0 = softmax cross entropy with hard-negative
 * mining: ssd_multibox_loss_box itself, the same launches, the same bits), float focal_alpha and float focal_gamma.
 * conf_mode 1: columns 0 .. C-2 of conf are one-against-all logits, column C-1 (the background column) is not read.  Matching, obj,
 * cls, n_pos and the ignore byte are unchanged; nothing is mined and neg_pos_ratio is not read.  For every prior that is not ignored
 * and every column c < C-1, with x = conf[i][p][c], t = (cls[i][p] == c), z = t ? x : -x, softplus(u) = max(u, 0) + log1p(exp(-|u|)):
 *   FL     = a_t exp(-gamma softplus(z)) softplus(-z),       a_t = t ? alpha : 1 - alpha, or 1 where alpha < 0
 *   dFL/dx = (t ? 1 : -1) a_t exp(-gamma softplus(z)) (-gamma sigmoid(z) softplus(-z) - sigmoid(-z))
 * (alpha_t (1 - p_t)^gamma times the binary cross entropy with logits; finite for every finite logit; the weight is differentiated,
 * not detached).  losses[1] = sum of FL / n_pos (norm_mode 0) or the sum (norm_mode 1), reduced in a fixed order: two calls give the
 * same bits.  dconf is the gradient of that value, +0.0 in column C-1 and in every row of an ignored prior; with dloc == dconf == NULL
 * only the losses are computed.  losses[0], losses[2], dloc, obj, cls and ign are those of conf_mode 0, bit for bit.
 * Five launches: the matching (no log-softmax), the per-image pass (no radix select), the finalize pass (dloc, losses[0], losses[2]),
 * a dense pass over conf (read once, dconf written once) and a one-block sum.  The workspace is ssd_multibox_loss's.
 * Errors: as ssd_multibox_loss_box; conf_mode outside 0 .. 1, focal_alpha > 1 or NaN, focal_gamma < 0, infinite or NaN are
 * SSD_ERR_BAD_SHAPE (in either conf_mode). */
size_t ssd_multibox_loss_focal_workspace(int bs, int P, int n_gt, int n_ign);
int ssd_multibox_loss_focal(const float* loc, const float* conf, const float* gt_boxes, const float* gt_classes,
                            const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh, const float* priors_xyxy,
                            int P, int n_classes, float iou_threshold, int neg_pos_ratio, int norm_mode, const float* ign_boxes,
                            const int32_t* ign_start, int n_ign, float ignore_threshold, int overlap_mode, int loc_mode,
                            int conf_mode, float focal_alpha, float focal_gamma, float* losses, int32_t* obj, int32_t* cls,
                            uint8_t* ign, float* dloc, float* dconf, void* workspace, size_t workspace_bytes, void* stream);
/* The dense pass of conf_mode 1 and its sum alone, launched as ssd_multibox_loss_focal launches them, for tests and tools: conf
 * (bs,P,n_classes), cls (bs,P) int32 class of every prior (n_classes - 1 = background), ign (bs,P) bytes (non-zero: the prior is ignored)
 * or NULL, n_pos > 0 the divisor of norm_mode 0.  conf_loss[0] receives what losses[1] receives there; dconf (bs,P,n_classes) may be
 * NULL.  workspace: 4 * bs * ceil(P / 128) bytes rounded up to a multiple of 256, 16-byte aligned.  Status codes in the order null,
 * shape (the rules of ssd_multibox_loss_focal; n_pos <= 0 or NaN), alignment, workspace. */
size_t ssd_focal_dense_workspace(int bs, int P);
int ssd_focal_dense(const float* conf, const int32_t* cls, const uint8_t* ign, int bs, int P, int n_classes, float n_pos, int norm_mode,
                    float focal_alpha, float focal_gamma, float* conf_loss, float* dconf, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ---- MultiBox loss with a choice of matching rule (ATSS, Zhang et al. 2020) ----------
 * ssd_multibox_loss_focal's arguments, meaning and status codes, plus int match_mode (0 = the IoU rule: ssd_multibox_loss_focal
 * itself, the same launches, the same bits; topk and the level description are then not looked at), int topk (1 .. 32), int n_levels
 * (1 .. 8) and two HOST arrays of n_levels ints: level_cells (grid cells of each pyramid level) and level_anchors (priors per cell).
 * The priors are stored level after level, cell after cell (row-major), the priors of a cell contiguous; sum cells * anchors = P.
 * match_mode 1, for every box g of an image:
 *   candidates  in every level the min(topk, cells) cells whose centre -- (cx, cy) of the cell's first prior -- is nearest to
 *               ((x1 + x2) / 2, (y1 + y2) / 2): squared f32 distance, nearest first, equal distances -> lower cell, NaN last; all
 *               priors of a chosen cell are candidates, in the order (level, rank of the cell, prior of the cell)
 *   statistics  IoU of each candidate with g (the matching's f32 op sequence); f64 mean and unbiased variance (0 for n < 2): lane j
 *               of 64 adds candidates j, j + 64, ... in order, then a butterfly (xor 32, 16, .. 1) adds the 64 partial sums
 *   accepted    d = (double)iou - mean: d >= 0 && d * d >= var (no square root), and the prior's centre strictly inside g
 *   conflicts   a prior accepted by several boxes of its image goes to the largest IoU bits, equal -> lower box index
 * A prior with a box is positive (class and regression target of that box); every other prior is background.  iou_threshold is not
 * read and there are no forced matches: a box can end with no prior and an image with no positive (its sel bytes are all zero).  A
 * batch without any positive divides by n_pos = 0 in norm_mode 0 exactly as the other entries do.  Everything behind the assignment
 * (mining, ignore bytes, loc and conf terms, norm modes) is unchanged.  obj of a non-positive prior is unspecified.
 * One memset node, the assignment pass (a workgroup per box) and the launches of ssd_multibox_loss_focal with the matching-free
 * instances of the first kernel.  No float atomics: two calls give the same bits.  The workspace is larger than the other entries'.
 * Errors: as ssd_multibox_loss_focal; match_mode outside 0 .. 1 is SSD_ERR_BAD_SHAPE; with match_mode 1 null level arrays are
 * SSD_ERR_NULL, and topk or n_levels out of range, a level with cells or anchors < 1 or levels that do not sum to P are
 * SSD_ERR_BAD_SHAPE. */
size_t ssd_multibox_loss_atss_workspace(int bs, int P, int n_gt, int n_ign);
int ssd_multibox_loss_atss(const float* loc, const float* conf, const float* gt_boxes, const float* gt_classes,
                           const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh, const float* priors_xyxy,
                           int P, int n_classes, float iou_threshold, int neg_pos_ratio, int norm_mode, const float* ign_boxes,
                           const int32_t* ign_start, int n_ign, float ignore_threshold, int overlap_mode, int loc_mode,
                           int conf_mode, float focal_alpha, float focal_gamma, int match_mode, int topk, int n_levels,
                           const int* level_cells, const int* level_anchors, float* losses, int32_t* obj, int32_t* cls,
                           uint8_t* ign, float* dloc, float* dconf, void* workspace, size_t workspace_bytes, void* stream);
/* The assignment pass of match_mode 1 alone, launched as ssd_multibox_loss_atss launches it, for tests and tools.  Outputs: assign
 * (bs,P) int32 global box index or -1; per box (each may be NULL) n_cand int32 candidates, mean / var float64, n_acc int32 accepted
 * candidates (before conflicts).  workspace: 8 * bs * P bytes rounded up to a multiple of 256, 16-byte aligned.  Status codes in the
 * order null, shape (bs <= 0, n_gt <= 0, P <= 0 or > 36000, the level rules above), alignment, workspace. */
size_t ssd_atss_assign_workspace(int bs, int P);
int ssd_atss_assign(const float* gt_boxes, const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh,
                    const float* priors_xyxy, int P, int topk, int n_levels, const int* level_cells, const int* level_anchors,
                    int32_t* assign, int32_t* n_cand, double* mean, double* var, int32_t* n_acc, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- decode + per-class NMS + top-k (Losses.py:11-98 inference; Util.py:86-96) ----------
 * l_ (P,4), c_ (P,n_classes) of ONE image, n_classes = conf width C, 2..256 (background = C-1 is never a detection).
 * Outputs (capacity top_k): boxes (top_k,4) xyxy scaled by (img_w,img_h,img_w,img_h), classes int64 (0..C-2), probs f32,
 * prior_ids int32, count int32[1].  Workspace: about 52 bytes per (class, prior, image) -- (C-1) * P candidate slots per image;
 * at P = 8732 and B = 32: 0.30 GB for C = 21, 1.17 GB for C = 81, 3.7 GB for C = 256. */
size_t ssd_decode_nms_workspace(int P, int n_classes);
int ssd_decode_nms(const float* l_, const float* c_, const float* priors_cxcywh, int P, int n_classes,
                   float min_score, float iou_threshold, int top_k, float img_w, float img_h,
                   float* boxes, int64_t* classes, float* probs, int32_t* prior_ids, int32_t* count,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Batched form: l_ (B,P,4), c_ (B,P,n_classes), img_wh (B,2) DEVICE floats
 * (img_w, img_h per image); outputs (B,top_k,...) and count (B).  One launch set for the whole batch. */
size_t ssd_decode_nms_batch_workspace(int B, int P, int n_classes);
int ssd_decode_nms_batch(const float* l_, const float* c_, const float* priors_cxcywh, const float* img_wh, int B, int P,
                         int n_classes, float min_score, float iou_threshold, int top_k, float* boxes, int64_t* classes,
                         float* probs, int32_t* prior_ids, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* Soft-NMS (Bodla et al. 2017) as the suppression rule of the same decode: the arguments of ssd_decode_nms[_batch] followed by
 * method (1 = linear, 2 = gaussian), sigma (> 0; gaussian only) and keep_score (1e-6 .. 1).  Per class, in descending order of
 * probability (ties: lower prior index): pick the live candidate with the largest score (ties: earlier in that order), stop once
 * it is below keep_score, otherwise emit it and multiply every other live score by
 *   linear:   iou > iou_threshold ? 1 - iou : 1          gaussian:   expf(-(iou * iou) / sigma)          1 where iou is not finite;
 * a candidate whose score falls below keep_score is dropped.  At most top_k picks per class; the emitted probs are the decayed
 * scores, and the cross-class top-k runs on them.  The same workspace as the hard rule, no allocation, no host synchronisation.
 * SSD_ERR_BAD_SHAPE -- before anything is enqueued -- for another method, sigma <= 0, keep_score or iou_threshold (0 .. 1) out of
 * range, or P > 40704 (the live scores of a class, 4 * P bytes, stay in LDS). */
int ssd_decode_nms_soft(const float* l_, const float* c_, const float* priors_cxcywh, int P, int n_classes,
                        float min_score, float iou_threshold, int top_k, float img_w, float img_h,
                        float* boxes, int64_t* classes, float* probs, int32_t* prior_ids, int32_t* count,
                        void* workspace, size_t workspace_bytes, void* stream, int method, float sigma, float keep_score);
int ssd_decode_nms_batch_soft(const float* l_, const float* c_, const float* priors_cxcywh, const float* img_wh, int B, int P,
                              int n_classes, float min_score, float iou_threshold, int top_k, float* boxes, int64_t* classes,
                              float* probs, int32_t* prior_ids, int32_t* count, void* workspace, size_t workspace_bytes, void* stream,
                              int method, float sigma, float keep_score);
/* The decode with a choice of score, for a model trained with the sigmoid focal term (ssd_multibox_loss_focal): the arguments of
 * ssd_decode_nms[_batch]_soft -- method 0 = the greedy rule (sigma and keep_score are then not read), 1 / 2 = Soft-NMS -- followed by
 * score_mode: 0 = softmax over the C columns (ssd_decode_nms[_batch][_soft] itself, the same launches), 1 = the probability of class
 * c in 0 .. C-2 is sigmoid(c_[.., c]), computed as 1 / (1 + exp(-|x|)), times exp(-|x|) where x < 0 (no overflow; exactly 1.0 for
 * large x); the value of the background column C-1 takes no part.  Everything after the score -- the candidate keys, their sort,
 * both suppression rules, the cross-class top-k -- is unchanged, as are the workspaces.  Another method or score_mode:
 * SSD_ERR_BAD_SHAPE. */
int ssd_decode_nms_score(const float* l_, const float* c_, const float* priors_cxcywh, int P, int n_classes,
                         float min_score, float iou_threshold, int top_k, float img_w, float img_h,
                         float* boxes, int64_t* classes, float* probs, int32_t* prior_ids, int32_t* count,
                         void* workspace, size_t workspace_bytes, void* stream, int method, float sigma, float keep_score, int score_mode);
int ssd_decode_nms_batch_score(const float* l_, const float* c_, const float* priors_cxcywh, const float* img_wh, int B, int P,
                               int n_classes, float min_score, float iou_threshold, int top_k, float* boxes, int64_t* classes,
                               float* probs, int32_t* prior_ids, int32_t* count, void* workspace, size_t workspace_bytes, void* stream,
                               int method, float sigma, float keep_score, int score_mode);
/* The first two stages of the decode alone, for tests and tools, launched exactly as the decode launches them: every prior's box and
 * class probabilities, the candidates prob >= min_score of every class but the last (NaN is not >=), and their sort.  l_ (B,P,4),
 * c_ (B,P,n_classes), priors_cxcywh (P,4); n_classes = 2..256, C1 = n_classes - 1, P <= 100000.  Outputs, caller-owned, in the layout
 * the three entries below consume: boxes (B,P,4) xyxy of every prior; cand_cnt (B, C1+1) candidates per (image, class), the last
 * entry of an image 0; and per (image, class) the first cand_cnt entries of s_boxes (B,C1,P,4), s_prob (B,C1,P) and s_idx (B,C1,P)
 * prior ids, in descending order of probability, lower prior index first among equal probabilities.  Slots past a class's count are
 * not written.  Priors per block: 256 while 256 rows of (n_classes | 1) floats fit 48 KB (n_classes <= 47), 128 while 128 such rows
 * do (<= 95), else 64.  clear_with_kernel: 0 clears the counters with a memset node, as ssd_decode_nms[_batch] does, 1 with a kernel,
 * as the Soft-NMS decode does.  l_, priors_cxcywh, boxes, s_boxes and workspace 16-byte aligned; workspace: the candidate keys,
 * 8 * B * C1 * P bytes rounded up to a multiple of 256. */
size_t ssd_decode_sorted_workspace(int B, int P, int n_classes);
int ssd_decode_sorted(const float* l_, const float* c_, const float* priors_cxcywh, int B, int P, int n_classes, float min_score,
                      float* boxes, float* s_boxes, float* s_prob, int32_t* s_idx, int32_t* cand_cnt, void* workspace,
                      size_t workspace_bytes, void* stream, int clear_with_kernel);
/* ssd_decode_sorted with score_mode as in ssd_decode_nms_score (0 is ssd_decode_sorted itself; another value: SSD_ERR_BAD_SHAPE) */
int ssd_decode_sorted_score(const float* l_, const float* c_, const float* priors_cxcywh, int B, int P, int n_classes, float min_score,
                            float* boxes, float* s_boxes, float* s_prob, int32_t* s_idx, int32_t* cand_cnt, void* workspace,
                            size_t workspace_bytes, void* stream, int clear_with_kernel, int score_mode);
/* The Soft-NMS kernel alone, for tests and tools: s_boxes (B,C1,P,4) xyxy and s_prob (B,C1,P) hold, per (image, class), the
 * cand_cnt[b * (C1 + 1) + c] candidates in descending order of probability (cand_cnt is (B, C1+1)); C1 = 1..255.  Outputs, per
 * (image, class) in pick order: kept_pos (B,C1,P) sorted positions, kept_prob (B,C1,P) decayed scores, kept_cnt (B, C1+1) number of
 * picks (<= max_picks, 1..4096).  Scores must be finite, positive and descending; anything else gives unspecified values, never an
 * access outside the arrays. */
int ssd_soft_nms_sorted(const float* s_boxes, const float* s_prob, const int32_t* cand_cnt, int B, int C1, int P, int method,
                        float iou_threshold, float sigma, float keep_score, int max_picks, int32_t* kept_pos, float* kept_prob,
                        int32_t* kept_cnt, void* stream);
/* The greedy rule's kernel alone, launched exactly as the decode launches it, for tests and tools: the layout of
 * ssd_soft_nms_sorted (cand_cnt[b * (C1 + 1) + c] <= P candidates per (image, class), in descending order of probability).  A kept
 * box suppresses every later box with IoU >= iou_threshold (f32, inter / ((area_a + area_b) - inter); NaN is not >=).  Outputs per
 * (image, class), in sorted order: kept_pos (B,C1,P) sorted positions of the survivors, kept_prob (B,C1,P) their probabilities
 * (the bits of s_prob), kept_cnt (B, C1+1) their number.  iou_threshold is passed through unchecked, as the decode passes it.
 * ssd_nms_plan (host only, no device needed) returns the launch decision for (B, C1, P): the block size (1024 where C1 * B <= 128,
 * else 512) and chunk_words; a class of n candidates is resolved 64 rows at a time while 64 * ceil(n / 64) <= chunk_words and 32 rows
 * at a time beyond.  SSD_ERR_BAD_SHAPE where the decode would refuse (P > 34752: 32 rows of all columns exceed the LDS). */
int ssd_nms_plan(int B, int C1, int P, int* threads, int* chunk_words);
int ssd_nms_sorted(const float* s_boxes, const float* s_prob, const int32_t* cand_cnt, int B, int C1, int P, float iou_threshold,
                   int32_t* kept_pos, float* kept_prob, int32_t* kept_cnt, void* stream);
/* The cross-class top-k of the decode alone, for tests and tools, on caller-made survivors: s_boxes (B,C1,P,4), s_idx (B,C1,P) prior
 * ids, and per (image, class) the first kept_cnt[b * (C1 + 1) + c] entries of kept_pos (positions into the class's P slots) and
 * kept_prob (positive probabilities); img_wh (B,2) device floats.  Outputs as ssd_decode_nms_batch (capacity top_k per image; slots
 * past count are not written).  All survivors in class-major order if at most top_k, else the top_k largest probabilities, ties in
 * class-major order, in descending order.  C1 = 1..255, top_k = 1..4096, P <= 100000; s_boxes, boxes and workspace 16-byte
 * aligned.  workspace: two arrays of 4 * B * C1 * P bytes, each rounded up to a multiple of 256. */
int ssd_topk_emit_sorted(const float* s_boxes, const int32_t* s_idx, const int32_t* kept_pos, const float* kept_prob,
                         const int32_t* kept_cnt, const float* img_wh, int B, int C1, int P, int top_k, float* boxes,
                         int64_t* classes, float* probs, int32_t* prior_ids, int32_t* count, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- mAP evaluator (Util.py:783-885 get_map: per-class 11-point interpolated AP, IoU > 0.5, one claim per
 * ground-truth box, no 'difficult' handling) over B images given as concatenated arrays:
 * det_* (D rows; det_start[B+1] = first row of each image), gt_* (G rows; gt_start[B+1]); classes are int32 in
 * [0, n_classes) (others are ignored, as the reference's `range(20)` loop does).  recall_levels is a HOST array
 * (the reference's torch.arange(0, 1.1, 0.1) as doubles), n_levels <= 16.  Outputs: tp (D bytes, must be zeroed by
 * the caller; 1 = true positive), table (n_classes x n_levels doubles: max precision at recall >= level, 0 where none;
 * AP[c] = mean of row c), counts (2*n_classes int32: detections per class, then ground truth per class). */
size_t ssd_map_eval_workspace(int D, int G);
int ssd_map_eval(const float* det_boxes, const int32_t* det_classes, const float* det_scores, const int32_t* det_start,
                 int D, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_start, int G, int B,
                 int n_classes, const double* recall_levels_host, int n_levels, uint8_t* tp, double* table,
                 int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- detection evaluator (Util.DetectionEvaluator; not in the reference): PASCAL VOC 'difficult' objects, up to 16 IoU
 * thresholds settled in ONE matching pass, 11- / 101-point and all-point AP with integer recall.
 * ssd_eval_match scores one batch of B images.  Detections are either concatenated (det_start[B+1], det_count NULL) or padded
 * (det_count[B], det_start NULL: image b owns rows b*K .. b*K + count[b] - 1 of the D = B*K rows; the rest is never read).
 * Ground truth is concatenated (gt_start[B+1]); gt_difficult (G bytes, 0/1) may be NULL = none difficult.  thresholds is a HOST
 * array of n_thresholds <= 16 ascending floats in (0, 1), compared as iou > thr.  Per detection, in descending (score, lower row
 * first) order inside its (image, class): the best-IoU box of ALL boxes of the class (first index on ties; any NaN IoU among
 * them = false positive) decides every threshold at once -- above = thresholds below that IoU; box difficult: ignored = above;
 * else tp = above & ~claimed[box], claimed[box] |= above.  Outputs per row: rec_classes (int32: the class, -1 = class outside
 * [0, n_classes), -2 = padding row), tp / ignored (uint16, bit t = thresholds[t]); n_gt (n_classes int32) is ADDED to: the
 * non-difficult boxes per class.  Start / count values are clamped to the arrays.
 * ssd_eval_ap orders D such rows per class (descending score, lower row first), drops the ignored ones per threshold and
 * writes, for n_levels = L in {10, 100}: out[(t*n_classes + c)*(L+1) + k] = max of cumTP/(cumTP+cumFP) over the positions with
 * cumTP*L >= k*n_gt (64-bit integers), 0 if none; for n_levels = 0: out[t*n_classes + c] = (sum over the true positives of the
 * running maximum of precision from the end) / n_gt, 0 where n_gt = 0.  n_det (n_classes int32) = rows per class. */
size_t ssd_eval_match_workspace(int G);
int ssd_eval_match(const float* det_boxes, const int32_t* det_classes, const float* det_scores, const int32_t* det_start,
                   const int32_t* det_count, int K, int D, const float* gt_boxes, const int32_t* gt_classes,
                   const uint8_t* gt_difficult, const int32_t* gt_start, int G, int B, int n_classes,
                   const float* thresholds_host, int n_thresholds, int32_t* rec_classes, uint16_t* tp, uint16_t* ignored,
                   int32_t* n_gt, void* workspace, size_t workspace_bytes, void* stream);
size_t ssd_eval_ap_workspace(int D);
int ssd_eval_ap(const int32_t* rec_classes, const float* det_scores, const uint16_t* tp, const uint16_t* ignored, int D,
                const int32_t* n_gt, int n_classes, int n_thresholds, int n_levels, double* out, int32_t* n_det,
                void* workspace, size_t workspace_bytes, void* stream);

/* ---- COCO evaluator (Util.CocoEvaluator; not in the reference): pycocotools' box protocol -- crowd regions, area ranges,
 * maxDets, AP and AR -- on up to 16 thresholds x 4 area ranges in ONE matching pass.
 * ssd_coco_match scores one batch of B images; detections and ground truth are laid out as for ssd_eval_match.  gt_crowd (G bytes,
 * 0/1) and gt_area (G floats) may be NULL = no crowd object / area (x2-x1)*(y2-y1) in float32.  thresholds (n_thresholds <= 16
 * ascending floats in (0, 1)), area_lo / area_hi (n_areas <= 4 inclusive bounds, lo <= hi) are HOST arrays; max_det_last in
 * 1..65535.  An object is ignored in range a if it is crowd or area < lo[a] or area > hi[a].  Per detection, in descending (score,
 * lower row first) order inside its (image, class), rank = its 0-based position; ranks >= max_det_last only get their rank.  At
 * every pair (a, t), each with its own claimed set: overlap = IoU (crowd object: intersection / detection area); candidates = the
 * class's objects unclaimed at (a, t), plus every crowd object, with overlap >= thresholds[t] (NaN never); the match is the best
 * non-ignored candidate, else the best ignored one, the later object on equal overlap, and becomes claimed; matched to a
 * non-ignored object -> tp, to an ignored one -> ignored, unmatched with the detection's own area outside [lo[a], hi[a]] ->
 * ignored.  Outputs per row: rec_classes (as ssd_eval_match), tp / ignored (uint64, bit a*16 + t), rank (int32, -1 = the row is in
 * no list); n_gt (n_areas x n_classes int32) is ADDED to: the non-ignored objects.  Workspace: one 64-bit claimed word per object.
 * ssd_coco_ap orders D such rows per class (descending score, lower row first) and, over the rows with rank < max_dets[M-1] that
 * are not ignored at (a, t), writes out[((t*n_areas + a)*n_classes + c)*101 + k] = max of cumTP/(cumTP+cumFP) over the positions
 * with cumTP*100 >= k*n_gt (64-bit integers), 0 if none; tp_count[((t*n_areas + a)*M + m)*n_classes + c] = true positives with
 * rank < max_dets[m] (HOST array of M <= 4 ascending values in 1..65535); n_det (n_classes int32) = rows per class. */
size_t ssd_coco_match_workspace(int G);
int ssd_coco_match(const float* det_boxes, const int32_t* det_classes, const float* det_scores, const int32_t* det_start,
                   const int32_t* det_count, int K, int D, const float* gt_boxes, const int32_t* gt_classes,
                   const uint8_t* gt_crowd, const float* gt_area, const int32_t* gt_start, int G, int B, int n_classes,
                   const float* thresholds_host, int n_thresholds, const float* area_lo_host, const float* area_hi_host,
                   int n_areas, int max_det_last, int32_t* rec_classes, uint64_t* tp, uint64_t* ignored, int32_t* rank,
                   int32_t* n_gt, void* workspace, size_t workspace_bytes, void* stream);
size_t ssd_coco_ap_workspace(int D);
int ssd_coco_ap(const int32_t* rec_classes, const float* det_scores, const uint64_t* tp, const uint64_t* ignored,
                const int32_t* rank, int D, const int32_t* n_gt, int n_classes, int n_thresholds, int n_areas,
                const int32_t* max_dets_host, int n_max_dets, double* out, int32_t* tp_count, int32_t* n_det,
                void* workspace, size_t workspace_bytes, void* stream);

/* ---- input pipeline (Dataset.py:10-13,24-39 Resize((300,300)) + ToTensor + Normalize; Util.py:610-749 expand /
 * random_crop / flip as geometry) on 8-bit HWC RGB images packed in one device arena.  The resize reproduces
 * Pillow's Image.resize(BILINEAR) on 8-bit images bit for bit.  Geometry per image, in this order: the source is
 * placed at (place_top, place_left) on a canvas_h x canvas_w canvas of `filler` (no expand: canvas = source, place
 * 0,0); the window (crop_top, crop_left, crop_h, crop_w) of the canvas is taken (no crop: the whole canvas); its
 * columns are mirrored when flip != 0; the result is resized to out_h x out_w and normalised into out_nchw
 * (B,3,out_h,out_w) float32.  descs_dev / descs_host are the same B descriptors in device / host memory. */
typedef struct ssd_image_desc {
    int64_t src_offset;            /* byte offset of the image's first pixel in the arena */
    int32_t src_h, src_w;
    int32_t canvas_h, canvas_w, place_top, place_left;
    int32_t crop_top, crop_left, crop_h, crop_w;
    int32_t flip, reserved;
} ssd_image_desc;
/* photometric_distort (Util.py:752-780) on the SOURCE images of the arena, in place, before ssd_preprocess_u8: up to four
 * ops per image in the image's own order; kind 0 brightness, 1 contrast, 2 saturation (alpha = the enhancement factor as
 * float32, Pillow's Image.blend argument), 3 hue (hue_delta = int(hue_factor * 255) & 255).  Bit-identical to the Pillow
 * arithmetic torchvision's PIL back end runs.  Host and device copies of both descriptor arrays, as for the resize. */
typedef struct ssd_photo_desc {
    int32_t n_ops;
    int32_t kind[4];
    float alpha[4];
    int32_t hue_delta[4];
} ssd_photo_desc;
size_t ssd_photometric_workspace(int B);
int ssd_photometric_u8(uint8_t* arena, const ssd_image_desc* descs_dev, const ssd_image_desc* descs_host,
                       const ssd_photo_desc* photo_dev, const ssd_photo_desc* photo_host, int B, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t ssd_preprocess_workspace(const ssd_image_desc* descs_host, int B, int out_h, int out_w);
int ssd_preprocess_u8(const uint8_t* arena, const ssd_image_desc* descs_dev, const ssd_image_desc* descs_host, int B,
                      int out_h, int out_w, const float* mean3_host, const float* std3_host, const uint8_t* filler3_host,
                      float* out_nchw, void* workspace, size_t workspace_bytes, void* stream);
/* The same resize / normalise pass into destination RECTANGLES: T tiles compose B output images (mosaic augmentation: four sources
 * per training image, each resized into one quadrant; a plain image is one full-frame tile).  Tile t is what ssd_preprocess_u8
 * computes for `src` at the output size (dst_h, dst_w) -- coefficients from crop_w / dst_w and crop_h / dst_h, so a tile never
 * samples another tile's source -- written to out[out_image][c][dst_top + oy][dst_left + ox].  The tiles of every output image
 * must cover it exactly once, so every output element is written once and nothing is cleared first.
 *   reserved[] carries where the tile's scratch lies in the workspace, in the packed order of the tile list:
 *     reserved[0] = sum of (dst_w + dst_h) over the tiles before t            (its first coefficient row)
 *     reserved[1] = sum of ceil(crop_h * dst_w * 3 / 256) over the tiles before t   (its intermediate rows, in 256-byte units)
 *     reserved[2] = 0
 *   The workspace query reads the geometry only; ssd_preprocess_tiles_u8 refuses descriptors whose reserved[] differ.
 * Refused before anything is enqueued, the first that applies: SSD_ERR_NULL (a NULL pointer); SSD_ERR_BAD_SHAPE (T, B, out_h or
 * out_w <= 0, T or B above 65535; out_image outside 0 .. B-1; dst_h or dst_w < 1 or a rectangle that leaves the output; anything
 * ssd_preprocess_u8 refuses of `src`, its tap bound -- a crop more than 31 times its rectangle, per axis -- taken against
 * dst_h / dst_w; tiles of one image that overlap, leave a gap, or an image without a tile; reserved[] not as above);
 * SSD_ERR_ALIGN (workspace not 16-byte aligned); SSD_ERR_WORKSPACE.  The query returns 0 for what would be refused for shape. */
typedef struct ssd_tile_desc {
    ssd_image_desc src;            /* source image, canvas, crop window, flip: as for ssd_preprocess_u8 */
    int32_t out_image;             /* 0 .. B-1 */
    int32_t dst_top, dst_left, dst_h, dst_w;   /* rectangle of the out_h x out_w output it fills */
    int32_t reserved[3];
} ssd_tile_desc;
size_t ssd_preprocess_tiles_workspace(const ssd_tile_desc* tiles_host, int T, int B, int out_h, int out_w);
int ssd_preprocess_tiles_u8(const uint8_t* arena, const ssd_tile_desc* tiles_dev, const ssd_tile_desc* tiles_host, int T, int B,
                            int out_h, int out_w, const float* mean3_host, const float* std3_host, const uint8_t* filler3_host,
                            float* out_nchw, void* workspace, size_t workspace_bytes, void* stream);
/* Random affine augmentation of the batch either call above made: out[b] = in[b] warped by the 2x3 matrix m0 .. m5 of image b, which
 * maps an OUTPUT pixel centre to input coordinates (the inverse of the forward map the host draws).  in / out are (B,3,H,W) float32
 * and distinct -- a gather, no workspace; mats_dev / mats_host are the same B x 6 float32 coefficients in device / host memory (the
 * library validates the host copy, the kernel reads the device copy); fill3_host is the NORMALISED filler, per channel
 * ((float)filler_u8[c] / 255.0f - mean[c]) / std[c] in float32 -- the expression of ssd_preprocess_u8's last pass -- read by value.
 * Output (ox, oy), all in float32, every operation rounded on its own, in exactly this association:
 *     fx = (float)ox + 0.5f;  fy = (float)oy + 0.5f
 *     sx = ((m0*fx + m1*fy) + m2) - 0.5f;   sy = ((m3*fx + m4*fy) + m5) - 0.5f
 *     live = sx > -1 && sx < (float)W && sy > -1 && sy < (float)H        (float compares: a NaN is not live)
 *     not live: out[c] = fill[c] for the three channels -- decided BEFORE any float -> int conversion
 *     x0 = floorf(sx); y0 = floorf(sy); ax = sx - x0; ay = sy - y0
 *     v00, v01, v10, v11 = in[c] at (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1); a tap outside the image reads fill[c]
 *     top = v00 + (v01 - v00)*ax;  bot = v10 + (v11 - v10)*ax;  out[c] = top + (bot - top)*ay
 * So the identity (1,0,0, 0,1,0) is a bit-exact copy, an integer translation an exact shifted copy with filler, a quarter turn of a
 * square frame an exact permutation, and the result is continuous across the border.
 * Refused before anything is enqueued, the first that applies: SSD_ERR_NULL (a NULL pointer; `stream` may be NULL);
 * SSD_ERR_BAD_SHAPE (B, H or W <= 0; B > 65535; H*W >= 2^31; in and out ranges that overlap; a coefficient of mats_host that is
 * not finite).  Only enqueues on `stream`: no synchronisation. */
int ssd_affine_warp_f32(const float* in_nchw, float* out_nchw, const float* mats_dev, const float* mats_host, int B, int H, int W,
                        const float* fill3_host, void* stream);

/* ---- baseline JPEG decode into the arena's pixel slots, ahead of the two calls above: what
 * PIL.Image.open(f).convert("RGB") returns (libjpeg's default path), bit for bit -- Huffman decode, dequantise + the "islow"
 * integer IDCT, "fancy" triangle chroma upsampling (plain replication where the down-sampled plane is at most two samples
 * wide, as libjpeg chooses), 16-bit fixed-point YCbCr -> RGB.  Scope: SOF0, 8-bit, one interleaved scan, 1 component or 3
 * components YCbCr with luma sampling 1x1 / 2x1 / 2x2 and chroma 1x1, restart intervals, width and height 1 .. 4096; the host
 * parser (Dataset.parse_jpeg) keeps everything else away from this call.
 *   One descriptor per image.  Offsets are bytes in `arena`: the entropy-coded data (from behind the SOS header to the marker
 * that ends it) and the pixel slot of dst_bytes >= height * width * 3 bytes, which receives HWC RGB.  Segment k of the image
 * (k = 0 .. n_segments-1) begins seg_offsets[seg_first + k] bytes into the entropy-coded data and ends two bytes -- its RSTn
 * marker -- before segment k+1 begins, the last one at stream_bytes; it starts at MCU k * restart_interval.  restart_interval
 * 0: one segment.  Tables: quant[t] in natural (row-major) order; Huffman table t = 0, 1 the DC tables 0, 1 and t = 2, 3 the AC
 * tables 0, 1, as bits[t][l-1] = codes of length l and huffval[t][0 .. n_huffval[t]), n_huffval 0 = absent; per component
 * the selectors quant_sel (0 .. 3), dc_sel and ac_sel (0 .. 1).  coef_offset / plane_offset are workspace offsets that the
 * workspace query fills in.
 *   Three kernels: entropy decode, one lane per restart segment, one workgroup per image (an image without restart markers is
 * decoded by ONE lane); dequantise + IDCT, eight lanes per block; upsample + colour, one lane per pixel.  Every loop of the
 * entropy decoder is bounded whatever the stream holds, and no store leaves the image's coefficient planes (csrc/jpeg_entropy.h).
 * status[b] (int32, device) is 0, or a mask of 1 (no such Huffman code), 2 (coefficient index above 63), 4 (segment ends before
 * its MCUs), 8 (fewer segments than the MCU count needs); an image with a non-zero status gets a slot of zeros.
 *   ssd_jpeg_decode_workspace fills coef_offset / plane_offset of descs_host[0 .. B) and returns the workspace size, 0 for a
 * descriptor outside the scope.  Upload the descriptors after it.  ssd_jpeg_decode_u8 validates EVERYTHING on the host copies
 * before it enqueues -- NULL pointers (SSD_ERR_NULL), geometry, selectors, Huffman tables that are no canonical code or hold
 * more than 256 values, segment offsets outside the stream or out of order, more segments than the MCU count allows, streams or
 * slots outside the arena or overlapping one another, slots below height * width * 3 bytes, workspace offsets that are not the
 * query's (SSD_ERR_BAD_SHAPE), a small workspace (SSD_ERR_WORKSPACE) -- and only enqueues on `stream`: no synchronisation.
 * stages: SSD_JPEG_ALL, or a subset of the three kernels for timing them one by one (the later ones read what the earlier ones
 * left in the workspace). */
#define SSD_JPEG_MAX_DIM 4096
#define SSD_JPEG_ENTROPY 1
#define SSD_JPEG_IDCT 2
#define SSD_JPEG_COLOUR 4
#define SSD_JPEG_ALL 7
typedef struct ssd_jpeg_desc {
    int64_t stream_offset, dst_offset, dst_bytes;
    int64_t coef_offset, plane_offset;
    int32_t stream_bytes;
    int32_t seg_first, n_segments, restart_interval;
    int32_t width, height, n_components, h_samp, v_samp;
    int32_t n_huffval[4];
    uint8_t quant_sel[4], dc_sel[4], ac_sel[4];
    uint16_t quant[4][64];
    uint8_t bits[4][16];
    uint8_t huffval[4][256];
} ssd_jpeg_desc;
size_t ssd_jpeg_decode_workspace(ssd_jpeg_desc* descs_host, int B);
int ssd_jpeg_decode_u8(uint8_t* arena, size_t arena_bytes, const ssd_jpeg_desc* descs_dev, const ssd_jpeg_desc* descs_host,
                       const int32_t* seg_offsets_dev, const int32_t* seg_offsets_host, int n_seg_offsets, int B,
                       int32_t* status, void* workspace, size_t workspace_bytes, int stages, void* stream);

/* ---- the same decode with MANY lanes per restart segment, for streams without restart markers (csrc/jpeg_split.hip; algorithm and
 * bounds in csrc/jpeg_split.h): each segment is de-stuffed into a copy in the workspace and cut into subsequences of subseq_bytes
 * bytes (a multiple of 4 in 8 .. 4096); every subsequence is walked speculatively, the states at the boundaries are repaired until
 * they stop changing -- one workgroup per image, at most as many rounds as the longest segment has subsequences -- and a write pass
 * stores the coefficients.  Pixels and status are those of ssd_jpeg_decode_u8, bit for bit; a segment shorter than one subsequence
 * is one lane as there.  Streams of more than 2^27 bytes are outside the scope.
 *   ssd_jpeg_decode_split_workspace fills coef_offset / plane_offset exactly as ssd_jpeg_decode_workspace does, keeps that layout in
 * front and puts the copies and the per-subsequence records behind it; 0 for anything outside the scope.  ssd_jpeg_decode_split_u8
 * runs every host-side validation of ssd_jpeg_decode_u8, and refuses a bad subseq_bytes (SSD_ERR_BAD_SHAPE) and a workspace below
 * the split query's (SSD_ERR_WORKSPACE), before it enqueues anything.  `stages` as above (SSD_JPEG_ENTROPY is all four kernels of
 * the entropy decode).  stats: NULL, or B x 4 int32 on the device: subsequences, repair rounds, subsequence walks of the
 * synchronisation, 0. */
size_t ssd_jpeg_decode_split_workspace(ssd_jpeg_desc* descs_host, int B, const int32_t* seg_offsets_host, int n_seg_offsets,
                                       int subseq_bytes);
int ssd_jpeg_decode_split_u8(uint8_t* arena, size_t arena_bytes, const ssd_jpeg_desc* descs_dev, const ssd_jpeg_desc* descs_host,
                             const int32_t* seg_offsets_dev, const int32_t* seg_offsets_host, int n_seg_offsets, int B,
                             int32_t* status, void* workspace, size_t workspace_bytes, int stages, void* stream, int subseq_bytes,
                             int32_t* stats);

/* ---- diagnostic: out32[2*xcc] = shader-clock counter, out32[2*xcc+1] = 100 MHz wall clock, for each of the (up to 16)
 * XCCs a block landed on; slots must be zeroed by the caller.  Two probes bracket a region: average shader MHz =
 * 100 * d(counter) / d(wall clock) per XCC. */
int ssd_clock_probe(uint64_t* out32, void* stream);

/* ---- diagnostic (host only): node count of a captured hipGraph_t and how many of the nodes are kernel launches -- what one replay of
 * the captured train step (ddp.GraphedTrainStep; the loop of train_function.py:80-95) stands for. */
int ssd_graph_node_counts(void* graph, int* kernel_nodes, int* total_nodes);

/* ---- fused SGD (train.py:53-55: momentum .9, weight decay 5e-4; bias lr 2x) on a flat buffer;
 * grad_scale multiplies the gradient first (1/n_pos_global in data-parallel runs).  Per element, each line rounded once:
 *   g' = fma(weight_decay, p, g * scale);  buf = first_step ? g' : (momentum * buf) + g';  p = fma(-lr, buf, p)
 * which is torch.optim.SGD's own rounding sequence, so the two stay bit-identical.  momentum == 0: call with first_step = 1. */
int ssd_sgd_momentum(float* param, const float* grad, float* momentum_buf, size_t n, float lr, float momentum,
                     float weight_decay, const float* grad_scale_dev, int first_step, void* stream);

/* ---- gradient-norm clipping and the non-finite step guard of the fused SGD step (torch.nn.utils.clip_grad_norm_, which a user of
 * the reference loop puts between train_function.py:94 `loss.backward()` and :95 `optimizer.step()`), without leaving the device.
 *
 * ssd_grad_norm_partials: one pass over grad[0..n) (f32, 16-byte aligned, n % 4 == 0, pads zero) that writes
 * ssd_grad_norm_slots(n) per-workgroup partials into partials[slot0 ...] (f64; slot_capacity = slots the buffer holds):
 *   norm_kind 0: sums of squares accumulated in f64 (the square of an f32 is exact there);
 *   norm_kind 1: max |g| widened to f64, NaN if the range holds a NaN.
 * The grid depends on n alone and every reduction runs in a fixed order without atomics: results are bitwise reproducible.
 *
 * ssd_grad_clip_finalize: one workgroup folds partials[0..n_slots) -- all ranges of the step -- in a fixed order and writes
 * state[0..5) (4-byte words of a block the caller zeroes once):
 *   state[0] total_norm = (float)(sqrt(S) * (double)pre_scale)  (kind 0)  or  (float)max * pre_scale  (kind 1); pre_scale_dev may
 *            be NULL (= 1; ddp.py passes 1 / n_pos_global, which the flat gradient buffer still lacks);
 *   state[1] clip_coef  = min(1, (1 / (total_norm + 1e-6f)) * max_norm), f32, each of the three operations rounded once (correctly
 *            rounded reciprocal), a NaN kept: the sequence clip_grad_norm_ executes for `max_norm / (total_norm + 1e-6)` -- torch
 *            divides a number by a tensor as reciprocal-times-number -- so equal norms give bit-equal coefficients;
 *            max_norm < 0: no clipping, clip_coef = 1;
 *   state[2] grad_scale = pre_scale * clip_coef (clip_coef itself without pre_scale): what ssd_sgd_momentum* take as grad_scale_dev;
 *   state[3] skip (int32) = guard != 0 and total_norm is Inf or NaN;   state[4] skipped_steps (int32) += skip.
 *
 * ssd_sgd_momentum_guarded: ssd_sgd_momentum, same arithmetic and rounding, that writes nothing at all -- neither parameters nor
 * momentum -- when *skip_dev != 0. */
int ssd_grad_norm_slots(size_t n);
int ssd_grad_norm_partials(const float* grad, size_t n, int norm_kind, double* partials, int slot0, int slot_capacity, void* stream);
int ssd_grad_clip_finalize(const double* partials, int n_slots, int norm_kind, float max_norm, const float* pre_scale_dev, int guard,
                           float* state, void* stream);
int ssd_sgd_momentum_guarded(float* param, const float* grad, float* momentum_buf, size_t n, float lr, float momentum,
                             float weight_decay, const float* grad_scale_dev, int first_step, const int* skip_dev, void* stream);

/* ---- device-resident learning-rate schedule and weight EMA of the fused SGD step: what a per-iteration scheduler (warm-up, multistep,
 * cosine) and an averaged copy of the weights add to the loop of train_function.py:80-95, with no host value that changes from step
 * to step -- so a captured step replays under any schedule.  Every kernel is compiled without floating-point contraction.
 *
 * Schedule state: a block of 2 + G 4-byte words the caller zeroes once:
 *   state[0] step (int32): optimizer steps actually taken;   state[1] ema_w (f32): the EMA weight of the current step;
 *   state[2 .. 2+G) lr[g] (f32): the learning rate of parameter group g for the current step.
 *
 * ssd_sgd_schedule_advance: one workgroup.  *skip_dev != 0 (skip_dev may be NULL): writes nothing.  Otherwise, with t = state.step:
 *   lr[g] = lr_table[g * T + min(t, T-1)]  (lr_table: G x T f32, row g = group g's rate at step 0 .. T-1; past the end the last holds);
 *   ema_w = (float)(1 - d_t) computed in f64 from IEEE add / subtract / divide only, d_t = ema_warmup ? min(ema_decay, (1+t)/(10+t))
 *           : ema_decay;  ema_decay < 0: no EMA, ema_w = 0;
 *   step  = t + 1.
 * No transcendental runs on the device: every schedule is a table the host built.  G <= 0, T <= 0 or ema_decay >= 1 / NaN:
 * SSD_ERR_BAD_SHAPE.
 *
 * ssd_sgd_momentum_sched: ssd_sgd_momentum with lr = *lr_dev -- the same arithmetic and rounding sequence for param and
 * momentum_buf -- that writes nothing when skip_dev != NULL and *skip_dev != 0.  ema != NULL: after the new p is formed (and not
 * re-read), in f32, three separately rounded operations, no fma:  d = p - e;  m = *ema_w_dev * d;  e = e + m.  ema == NULL: no EMA
 * (ema_w_dev may then be NULL).  Ranges that are all 16-byte aligned with n % 4 == 0 move as 16-byte accesses, anything else
 * takes a scalar loop with the same results.  The grid is min(ceil(units / 256), 2048) workgroups of 256 threads, units = n / 4 (vector)
 * or n (scalar).
 *
 * ssd_swap_f32: a[i] <-> b[i] for two DISJOINT ranges (overlap: SSD_ERR_BAD_SHAPE); the same vector / scalar choice.
 *
 * All three only enqueue on `stream` (graph-capturable); n == 0 is SSD_OK.  Errors: SSD_ERR_NULL for a missing state, lr_table, param,
 * grad, momentum_buf, lr_dev, a or b, and for ema given without ema_w_dev; SSD_ERR_ALIGN for any pointer (skip_dev included) that is
 * not 4-byte aligned -- 16-byte alignment is never required, it only selects the vector form. */
int ssd_sgd_schedule_advance(void* state, const float* lr_table, int G, int T, double ema_decay, int ema_warmup, const int* skip_dev,
                             void* stream);
int ssd_sgd_momentum_sched(float* param, const float* grad, float* momentum_buf, float* ema, size_t n, const float* lr_dev,
                           const float* ema_w_dev, float momentum, float weight_decay, const float* grad_scale_dev, int first_step,
                           const int* skip_dev, void* stream);
int ssd_swap_f32(float* a, float* b, size_t n, void* stream);

/* ---- fused Adam / AdamW step on the same flat ranges and the same device words (learning rate, EMA weight, clip scale, skip flag) as
 * ssd_sgd_momentum_sched.  Compiled without floating-point contraction; every fused multiply-add below is an explicit one.
 *
 * Adam state: a block of its own (the schedule block above is unchanged) of three 8-byte words, 8-byte aligned, that the caller
 * initialises once to {1.0, 1.0, 0}:
 *   state[0] pow1 (f64): beta1^t as a running product;   state[1] pow2 (f64): beta2^t as a running product;
 *   state[2] low 4 bytes step (int32): Adam steps actually taken, t; high 4 bytes spare (zero).
 *
 * ssd_adam_advance: one workgroup.  *skip_dev != 0 (skip_dev may be NULL): writes nothing.  Otherwise step = t + 1, pow1 = pow1 * beta1,
 * pow2 = pow2 * beta2: one IEEE f64 multiply each per step, so the block after t steps is what t multiplications starting from 1.0 give
 * on any IEEE machine -- no pow() is involved, and a checkpointed counter restores the block bit for bit.
 *
 * ssd_adam_step, per element of n-element ranges, all f32, after ssd_adam_advance has run for this step (fma = one rounding):
 *   rate = lr_dev ? (double)*lr_dev : lr                                           (f64)
 *   g  = grad * *grad_scale_dev                                                    (only when grad_scale_dev is given)
 *   decoupled == 0 (Adam, L2):   g = fma(wd, p, g)                                 (weight_decay != 0; wd = (float)weight_decay)
 *   decoupled != 0 (AdamW):      p = p * (float)(1 - rate * weight_decay)          (weight_decay != 0; the factor formed in f64)
 *   m  = fma((float)(1 - beta1), g - m, m)
 *   v  = fma((float)(1 - beta2) * g, g, v * (float)beta2)
 *   den = sqrt(v) / (float)sqrt(1 - pow2) + (float)eps
 *   p  = p + ((float)(-(rate / (1 - pow1))) * m) / den
 * 1 - beta, the bias corrections, the division and the square root of the step size are f64 and rounded to f32 once each (one
 * division and one square root per thread, none per element); sqrt and / per element are correctly rounded f32.  That is
 * torch.optim.Adam / AdamW (foreach=False) with bit-equal exp_avg and exp_avg_sq; how far p is from torch's after one step is recorded
 * in tests/golden/adam_ref_distance.json.  ema != NULL: then the three operations of ssd_sgd_momentum_sched on the new p.
 * *skip_dev != 0: nothing at all is written.  Vector / scalar choice and grid as ssd_sgd_momentum_sched; gradient, moments and EMA
 * move through non-temporal 16-byte accesses, the parameters through plain ones.
 *
 * Both only enqueue on `stream` (graph-capturable).  Refusals, in this order: SSD_ERR_NULL for a missing state, param, grad, exp_avg or
 * exp_avg_sq and for ema given without ema_w_dev; SSD_ERR_BAD_SHAPE for a beta outside [0, 1), a negative (or NaN) eps or weight_decay,
 * and a negative lr when lr_dev is NULL; SSD_ERR_ALIGN for a state that is not 8-byte aligned or any other pointer that is not 4-byte
 * aligned; then n == 0 is SSD_OK. */
int ssd_adam_advance(void* state, double beta1, double beta2, const int* skip_dev, void* stream);
int ssd_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, size_t n, double lr, const float* lr_dev,
                  const float* ema_w_dev, const void* state, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                  const float* grad_scale_dev, const int* skip_dev, void* stream);

/* ---- BatchNorm2d in training mode, Dropout / Dropout2d (SSD_resnet34 train mode: Model.py:24,56-70,72-126 and
 * torchvision's BasicBlock).  Tensors are [M][ld] f32 rows whose first C columns are the channels (M = N*H*W), C % 4 == 0,
 * ld % 4 == 0, rows 16-byte aligned.  Reductions use fixed-order slab partials (no atomics): results are bitwise reproducible.
 *
 * Dropout generator: Philox4x32-10 with key = {lo32(seed), hi32(seed)}; element idx of site `site` reads word (idx & 3) of
 * philox({lo32(idx >> 2), hi32(idx >> 2), site, 0}) and is kept iff (word >> 8) * 2^-24 < 1 - p (float); kept values are scaled by
 * 1/(1-p).  drop_mode 0: none; 1: elementwise nn.Dropout, idx = row*C + c; 2: nn.Dropout2d per (sample, channel),
 * idx = n*C + c with n = row / HW. */

/* workspace bytes of ssd_bn_train_stats / ssd_bn_train_bwd for M rows of C channels */
size_t ssd_bn_workspace(size_t M, int C);

/* batch mean and biased variance over the M rows (Welford per thread, Chan merges in a fixed order); writes mean, invstd =
 * 1/sqrt(var+eps), scale = gamma*invstd, shift = beta - mean*scale (C floats each), updates running_mean / running_var (unbiased
 * variance, `momentum` weight) and num_batches_tracked += 1 when those are non-NULL.  gamma / beta NULL: 1 / 0.  M >= 2. */
int ssd_bn_train_stats(const float* x, int ldx, size_t M, int C, const float* gamma, const float* beta, float eps, float momentum,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd,
                       float* scale, float* shift, void* workspace, size_t workspace_bytes, void* stream);

/* y = drop( act( x*scale + shift [+ res*res_scale + res_shift  |  + res] ) ), act = ReLU if relu; res / res_scale / res_shift may
 * be NULL (res_scale and res_shift together).  x may alias y (in place). */
int ssd_bn_apply(const float* x, int ldx, size_t M, int C, const float* scale, const float* shift, const float* res, int ldr,
                 const float* res_scale, const float* res_shift, int relu, int drop_mode, float p, uint64_t seed, int site, int HW,
                 float* y, int ldy, void* stream);

/* Backward of y = drop(BN(x)): g = dy * dropout factor, xhat = (x - mean)*invstd (mean / invstd from ssd_bn_train_stats);
 * sums[0..C) = sum g (dbeta), sums[C..2C) = sum g*xhat (dgamma); dgamma / dbeta (optional) written, or added to if accumulate;
 * dx (optional, may alias dy) = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)), zeroed where x <= 0 if relu_mask (the BatchNorm
 * follows a ReLU and x is its output). */
int ssd_bn_train_bwd(const float* dy, int ldd, const float* x, int ldx, size_t M, int C, const float* mean, const float* invstd,
                     const float* gamma, int drop_mode, float p, uint64_t seed, int site, int HW, int relu_mask, float* sums,
                     float* dgamma, float* dbeta, int accumulate, float* dx, int lddx, void* workspace, size_t workspace_bytes,
                     void* stream);

/* out[i] = 1 if dropout index i of (seed, site) is kept, else 0; n % 4 == 0.  A testing aid: the masks a forward used. */
int ssd_dropout_mask(uint8_t* out, size_t n, float p, uint64_t seed, int site, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_GFX950_H */
