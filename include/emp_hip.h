/*
 * emp_hip.h -- C ABI of libemp_hip.so, the MI355X (gfx950) implementation of empanada's
 * orthoplane-inference post-processing hot path.
 *
 * The reference (volume-em/empanada) is 100 % Python: it has no FFI.  This ABI is therefore
 * NEW surface; each entry point names the reference function(s) (path:line relative to the
 * reference root) whose arithmetic it replaces.  The Python package `empanada_amd` binds these
 * with ctypes (empanada_amd/_hip.py) behind the reference's own engine / matcher / tracker
 * names; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every pointer is a DEVICE pointer unless the name ends in _host.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and never allocates, frees or synchronises, so callers may capture it in a
 *     hipGraph.  Workspaces are caller-provided.
 *   - return value: 0 on success, negative EMP_E* on error; emp_last_error() returns a
 *     per-thread message.  No exceptions cross the boundary.
 *   - images are row-major; a "stack" is D slices of (H, W); "HW" = H*W.
 *   - labels: pan = class_id * label_divisor + instance_id (reference convention).
 */
#ifndef EMP_HIP_H
#define EMP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMP_OK 0
#define EMP_EINVAL (-1)   /* bad argument (shape, size, unsupported parameter) */
#define EMP_ELAUNCH (-2)  /* HIP launch / runtime error */
#define EMP_ENODEV (-3)   /* no usable gfx950 device */

#define EMP_MAX_KS 11       /* median kernel sizes 1,3,...,11 (reference: scripts/pdl_inference3d.py:28) */
#define EMP_MAX_CLASSES 16  /* semantic channels C, and class ids < 16 */
#define EMP_MAX_CENTERS 4096 /* per-slice centre capacity the in-LDS sort supports */
#define EMP_CENTER_LIMIT 65535 /* hard per-slice centre limit: ids and candidate lists are uint16 */

int emp_version(void);
const char *emp_last_error(void);
/* Number of visible HIP devices (does not create a context). */
int emp_device_count(void);

/* ---- D0: slice feeder: uint8 volume -> normalised, zero-padded fp32 model input ---------------------
 * replaces VolumeDataset.__getitem__ + albumentations Normalize + factor_pad for a device-resident volume
 *          empanada/data/volume_dataset.py:7-53, inference/postprocess.py:25-36 (factor_pad)
 * Slice s, row r, column c of the chosen plane is vol[s*stride_slice + r*stride_row + c*stride_col] (element
 * strides; xy: (H*W, W, 1), xz: (W, H*W, 1), yz: (1, H*W, W) for a (D,H,W) volume), so no transposed copy of the
 * volume is ever made.  out (n_slices, 1, hp, wp) fp32 = (x - mean255) * inv_std255 (two fp32 roundings, the
 * arithmetic of albumentations' Normalize with max_pixel_value = 255), rows >= h and columns >= w zero.       */
int emp_slices_to_input(const uint8_t *vol, int64_t stride_slice, int64_t stride_row, int64_t stride_col,
                        int n_slices, int h, int w, int hp, int wp, float mean255, float inv_std255,
                        float *out, void *stream);

/* ---- D0 with in-plane down-sampling: uint8 volume -> resized, normalised, zero-padded fp32 input ----
 * replaces VolumeDataset(scale = N).__getitem__: resize_by_factor (cv2.resize to (ceil(w/N), ceil(h/N)), default
 *          interpolation), then Normalize and factor_pad
 *          empanada/data/volume_dataset.py:45-51, empanada/data/utils/transforms.py:9-21
 * vol, the strides, n_slices, (h, w), mean255, inv_std255, out and stream as in emp_slices_to_input.  (dh, dw): the
 * resized plane, 1 <= dh <= h, 1 <= dw <= w; out is (n_slices, 1, hp, wp) with hp >= dh, wp >= dw, rows >= dh and
 * columns >= dw zero.  The resize is integer arithmetic on tables the host computes once per (source, destination)
 * length (empanada_amd.data.resize_tables; the fp32 coefficient arithmetic is never done on the device):
 *   row_off (dh) int32, row_coef (dh, 2) int16: first source row y0 and the 11-bit weights (b0, b1) of rows y0 and
 *   min(y0 + 1, h - 1);  col_off (dw) int32, col_coef (dw, 2) int16: the same for columns (a0, a1).
 *   area == 0:  r[y] = src[y][x0] * a0 + src[y][x1] * a1  (int32)
 *               u = (((b0 * (r[y0] >> 4)) >> 16) + ((b1 * (r[y1] >> 4)) >> 16) + 2) >> 2
 *   area != 0 (needs h == 2 dh and w == 2 dw, the tables are not read):
 *               u = (src[2r][2c] + src[2r][2c+1] + src[2r+1][2c] + src[2r+1][2c+1] + 2) >> 2
 * and out = ((float)u - mean255) * inv_std255.  Table offsets are clamped to the plane on the device.             */
int emp_slices_to_input_scaled(const uint8_t *vol, int64_t stride_slice, int64_t stride_row, int64_t stride_col,
                               int n_slices, int h, int w, int dh, int dw, int hp, int wp, const int32_t *row_off,
                               const int16_t *row_coef, const int32_t *col_off, const int16_t *col_coef, int area,
                               float mean255, float inv_std255, float *out, void *stream);

/* ---- D1 epilogue: fused BatchNorm(eval) + residual + ReLU on NHWC fp32 activations -----------------
 * replaces the elementwise tail of every conv block of the dense path:
 *          Bottleneck / BasicBlock forward         empanada/models/encoders/resnet.py:66-82,110-128
 *          conv_bn_act / separable_conv_bn_act     empanada/models/blocks.py:121-171
 * out[p, c] = act(x[p, c] * scale[c] + shift[c] (+ residual[p, c])), act = ReLU if relu != 0.
 * scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale (precomputed by the host).
 * x, residual: (n_pixels, C) fp32 (NHWC memory), C % 4 == 0, 16-byte aligned.  out: pixel p starts at
 * out + p * out_pixel_stride (floats; 0 means C): either dense (may alias x) or a channel slice of a wider NHWC
 * buffer, which is how the torch.cat of ASPP / decoder branches (aspp.py:96-101,
 * decoders/panoptic_deeplab.py:76-77) is written in place.                                                  */
int emp_bn_act_nhwc(const float *x, const float *scale, const float *shift, const float *residual,
                    int relu, int64_t n_pixels, int C, float *out, int64_t out_pixel_stride, void *stream);

/* ---- D2: depthwise k x k convolution on NHWC fp32 activations (stride 1, zero "same" padding) -------
 * replaces the depthwise half of SeparableConv2d   empanada/models/blocks.py:15-33
 *          (decoder fuse stages                     empanada/models/decoders/panoptic_deeplab.py:52-60,
 *           head trunks                             empanada/models/heads.py:9-19)
 * y[n, r, c, ch] = bias[ch] + sum_{i, j} x[n, r + i - k/2, c + j - k/2, ch] * w_kkc[(i * k + j) * C + ch]
 * evaluated as one fp32 FMA chain over the taps in raster order (i, then j) starting from +0; taps outside the
 * image contribute fma(0, w, acc).  x, y: (N, H, W, C) fp32; w_kkc: (k*k, C) (the (C, 1, k, k) Conv2d weight
 * transposed); bias: (C) or NULL; k in {3, 5}; C % 4 == 0; all pointers 16-byte aligned; y must not alias x. */
int emp_dwconv_nhwc(const float *x, const float *w_kkc, const float *bias, int N, int H, int W, int C,
                    int k, float *y, void *stream);

/* ---- D3: bilinear up-sampling with align_corners = True on fp32 activations ------------------------
 * replaces F.interpolate(..., mode='bilinear', align_corners=True) in
 *          PanopticDeepLab.forward (x4 heads)       empanada/models/panoptic_deeplab.py:100-113
 *          PanopticDeepLabDecoder.forward           empanada/models/decoders/panoptic_deeplab.py:70-78
 *          ASPPPooling.forward                      empanada/models/decoders/aspp.py:48-52
 * x: logical (N, C, h, w), y: logical (N, C, H, W), both addressed through 4 element strides (n, c, h, w), so
 * either side may be NCHW, NHWC or a channel slice of a wider NHWC buffer (the caller's torch.cat target).
 * src = dst * (in - 1) / (out - 1) in fp32 (0 when out == 1); i0 = floor(src), l = src - i0, i1 = min(i0+1, in-1);
 * y = (1-ly) * ((1-lx) * v00 + lx * v01) + ly * ((1-lx) * v10 + lx * v11), every operation a separate fp32
 * rounding.  x_strides / y_strides: HOST arrays of 4 int64.                                                 */
int emp_upsample_bilinear(const float *x, int N, int C, int h, int w, const int64_t *x_strides,
                          float *y, int H, int W, const int64_t *y_strides, void *stream);

/* ---- D4: convolution + BatchNorm(eval) + residual + ReLU in one kernel, NHWC fp32, fp32 matrix cores -----
 * replaces Conv2d -> BatchNorm2d -> (+ identity) -> ReLU chains of the dense path:
 *          Bottleneck / BasicBlock forward         empanada/models/encoders/resnet.py:66-82,110-128
 *          conv_bn_act, ASPP branches, projections empanada/models/blocks.py:121-171, decoders/aspp.py:22-102
 * out[p, co] = act(acc[p, co] * scale[co] + shift[co] + residual[p, co]); scale / shift / residual optional (NULL),
 * act = ReLU if relu != 0; acc = sum over taps (ky, kx) and input channels of x[n, oy*stride - pad + ky*dil,
 * ox*stride - pad + kx*dil, c] * w_okkc[co, ky, kx, c], evaluated as ONE fp32 fma chain from +0 (the MFMA is
 * bit-for-bit an fmaf chain): taps in raster order; per tap, slabs of S channels ascending; per slab the order
 * c, c + S/2 for c = 0..S/2-1; taps outside the image enter as x = 0.  S = emp_conv_k_slab(M = N*OH*OW,
 * Cout, 1, residual != NULL): 16 (three resident blocks per CU) when the launch has more than 512 blocks and does
 * not use the residual-prefetch variant, else 32.  has_residual means a residual the kernel can PREFETCH (16-byte
 * aligned, pixel stride a multiple of 4): a launch whose residual is not sums in the slab of has_residual = 0.  The
 * epilogue's multiply and adds are separate fp32 roundings, as in emp_bn_act_nhwc.
 * x: (N, H, W, Cin), Cin % 16 == 0; w_okkc: (Cout, KH, KW, Cin) (the Conv2d weight permuted); residual and out
 * are addressed as base + pixel * pixel_stride + co (stride 0 means Cout), so out may be a channel slice of a
 * wider NHWC concat buffer.  x and w 16-byte aligned; out must not alias x.                                    */
int emp_conv_k_slab(int64_t M, int Cout, int batch, int has_residual);
/* the same for a given Cin: Cin % 32 != 0 (RegNet widths 144, 1296: multiples of 16 only) always takes S = 16 */
int emp_conv_k_slab_cin(int64_t M, int Cout, int batch, int has_residual, int Cin);
/* D4b: short-K pointwise layers (1x1, stride 1, no padding, Cin 64 or 128, Cout a multiple of 128, at least 65 536
 * output pixels: conv3 + identity and the shortcut projection of the ResNet bottleneck's layer1 / layer2,
 * empanada/models/encoders/resnet.py:98-118) are computed by a weight-stationary kernel inside emp_conv_bn_act_nhwc
 * (emp_conv1x1.hip: weights resident in LDS, activations straight into the MFMA operands, epilogue from the
 * accumulators).  Its summation order is the D4 order with a K-slab of 64: slabs of 64 channels ascending, inside a
 * slab j = 0..31: channel j, then channel 32 + j.  emp_conv_k_slab_geom returns the slab emp_conv_bn_act_nhwc will use
 * for a given geometry (64 for these layers, else emp_conv_k_slab_cin's answer); relu as in emp_conv_bn_act_nhwc.
 * The same kernel also takes, from 262 144 output pixels on and without a residual, the bottleneck's conv1 shapes
 * 256 -> 64, 64 -> 64 and 256 -> 128, and inside emp_gemm_nt_batched the GEMMs with K and N in {64, 128} and
 * batch * M >= 262 144 (the Winograd F(4x4,3x3) GEMMs of layer1 / layer2).  For THESE it sums in the order of the tiled
 * kernel (K-slab emp_conv_k_slab_cin / emp_conv_k_slab, 16 at such sizes), so the result does not depend on which
 * kernel ran and emp_conv_k_slab* answer as before.  emp_conv1x1_ws_eligible: 1 for every convolution geometry the
 * kernel takes without a residual (for the conv1 shapes: given no residual); EMP_CONV_NO_WS=1 in the environment turns
 * all of it off.
 * Kind 3: 1x1, stride 1, no padding, Cin == 256, Cout a multiple of 128 up to 1024, at least 65 536 output pixels and
 * at least 8 * 65 536 / (Cout / 128) of them (sixteen 32-pixel tiles for every wave of the persistent grid), WITH
 * a residual and relu in {0, 1} (layer3's conv3 + identity, 256 -> 1024) also runs on the weight-stationary kernel --
 * when residual, out, scale and shift are 16-byte aligned, both pixel strides are multiples of 4 below 2^24, and the
 * tiled kernel's plan for the call is its residual-prefetch variant (K-slab 32).  It sums in THAT order (slabs of 32
 * channels ascending, inside a slab j = 0..15: channel j, then channel 16 + j), so the result does not depend on which
 * kernel ran and emp_conv_k_slab_geom keeps answering 32.  Without a residual these shapes stay on the tiled kernel.
 * emp_conv1x1_ws_kind_for: the kind (0: tiled kernel; 1: the 64-slab shapes; 2: the conv1 shapes; 3) a call of that
 * geometry with / without a residual takes, given aligned operands.  EMP_CONV_NO_WS3=1 turns kind 3 alone off
 * (experiments: A/B against the tiled kernel). */
int emp_conv_k_slab_geom(int64_t M, int Cout, int has_residual, int Cin, int KH, int KW, int stride, int pad, int relu);
int emp_conv1x1_ws_eligible(int64_t M, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu);
int emp_conv1x1_ws_kind_for(int64_t M, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu, int has_residual);
/* number of weight-stationary launches emp_conv_bn_act_nhwc has made so far in this process for kind 1, 2 or 3 (-1 for
 * another kind): the dispatch also depends on alignment, pixel strides and the tiled plan, which the queries above do
 * not see, so this is how a test tells which kernel a call took. */
int64_t emp_conv1x1_ws_launches(int kind);
/* D4c: the GEMM-shaped launches of the tiled kernel (1x1, stride 1, no padding, no residual, relu in {0, 1}, Cout a
 * multiple of 128, plan: K-slab 16 and 128-wide tiles; emp_conv_bn_act_nhwc with scale AND shift, and emp_gemm_nt_batched)
 * run on a persistent form of it (emp_conv_stream.hip) once the launch has at least 2 048 tiles of 128 x 128 (8/3 for
 * each of its 768 resident blocks, three per CU): a block walks a sequence of tiles with one slab stream across them and
 * stores from the accumulators.  Same summation order and epilogue arithmetic, so the result does not depend on which
 * kernel ran and emp_conv_k_slab* answer as before.  emp_conv_stream_eligible: 1 = a launch of that geometry takes it,
 * given 16-byte-aligned operands and pixel strides that are multiples of 4 (batch > 1: emp_gemm_nt_batched with M rows,
 * K = Cin, N = Cout; proj != 0: emp_conv_bn_act_proj_nhwc, never eligible); 0 for the geometries of the
 * weight-stationary kernels.  EMP_CONV_NO_STREAM=1 in the environment turns it off (experiments: A/B).
 * emp_conv_stream_grid: blocks of a launch of batch x tiles tiles.  emp_conv_stream_walk: 1 and the (entry, tile) --
 * tile = pixel tile * cout tiles + cout tile -- block `block` of `grid` blocks works on in its step `step`, 0 when
 * the block has no such step; block b only visits tiles of the contiguous eighth of the sequence that XCD b & 7 owns.
 * emp_conv_stream_launches: launches of the persistent kernel so far in this process.                            */
int emp_conv_stream_eligible(int batch, int64_t M, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu,
                             int has_residual, int proj);
int emp_conv_stream_grid(int64_t tiles, int batch);
int emp_conv_stream_walk(int64_t tiles, int batch, int grid, int block, int64_t step, int64_t *entry, int64_t *tile);
int64_t emp_conv_stream_launches(void);
/* relu == 2 selects the squeeze-excite gate epilogue (SqueezeExcite.forward, empanada/models/blocks.py:35-50:
 * x * sigmoid(conv(s) + bias)): out = residual * (1 / (1 + expf(-(acc * scale + shift)))), residual = the gated
 * tensor x (required); the division and the product are separate fp32 roundings, expf is the device library's;
 * its K-slab is emp_conv_k_slab_cin(M, Cout, 1, 0, Cin) (the residual-prefetch variant is never used for it).
 * Cin % 16 == 0 (round 2; was 32).                                                                            */
int emp_conv_bn_act_nhwc(const float *x, const float *w_okkc, const float *scale, const float *shift,
                         const float *residual, int64_t res_pixel_stride, int relu, int N, int H, int W,
                         int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, float *out,
                         int64_t out_pixel_stride, void *stream);
/* D4c: the same convolution for SMALL launches (one 512^2 tile at batch 1: layer3 / layer4 / ASPP have 8-64 tiles of 128
 * pixels for 256 CUs) -- the per-slice protocol's forward, empanada/inference/engines.py:141-159 one image per call.
 * The reduction over the S = KH KW Cin / 32 slabs of 32 channels is cut into k_splits ranges [S z / k, S (z + 1) / k);
 * every range is a block of its own and writes its partial sums (the fmaf chain of emp_conv_bn_act_nhwc with K-slab 32,
 * from +0) to plane z of `work` (k_splits x N*OH*OW x Cout floats); a second pass adds the planes in ascending order
 * and applies the epilogue, out = relu?(sum * scale + shift (+ residual)), every operation a separate fp32 rounding.
 * Deterministic.  Cin % 32 == 0, Cout % 4 == 0, relu 0 / 1; all pointers 16-byte aligned, pixel strides % 4 == 0.
 * emp_conv_splitk_plan: the number of ranges worth using for a geometry (1 = the launch fills the chip as it is). */
int emp_conv_splitk_plan(int64_t M, int Cout, int Cin, int KH, int KW);
int emp_conv_splitk_bn_act_nhwc(const float *x, const float *w_okkc, const float *scale, const float *shift,
                                const float *residual, int64_t res_pixel_stride, int relu, int N, int H, int W,
                                int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, int k_splits,
                                float *work, float *out, int64_t out_pixel_stride, void *stream);

/* D4 + D6 in one launch: the convolution's epilogue also evaluates a following 1x1 convolution to proj_n <= 4
 * channels (head = separable conv -> BN -> ReLU -> Conv2d(256, n, 1): heads.py:9-19), so the 256-channel activation
 * is neither written nor re-read (out may be NULL).  proj_out (N, proj_n, OH*OW) planar, ZEROED by the caller;
 * bias is the caller's to add.  Per output pixel and q: for each cout tile (128 wide) the 32 lanes of the row hold
 * ((v0 w0 + v1 w1) + v2 w2) + v3 w3 over their 4 couts (products and sums separate fp32 roundings), summed over
 * the lanes in ascending cout order (left fold), and the tile sums are added to proj_out with one atomicAdd each
 * (Cout is 128 or 256: with at most two tiles the result is independent of their order).                      */
int emp_conv_bn_act_proj_nhwc(const float *x, const float *w_okkc, const float *scale, const float *shift,
                              int relu, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                              int pad, int dil, const float *proj_w, int proj_n, float *proj_out,
                              float *out, int64_t out_pixel_stride, void *stream);

/* ---- D8: grouped 3x3 convolution + BatchNorm(eval) + ReLU, NHWC fp32, fp32 matrix cores (16x16x4 tiles) -----
 * replaces Conv2d(w, w, 3, stride, padding=1, groups=w/group_w) -> BatchNorm2d -> ReLU of the RegNet bottleneck
 *          Bottleneck.__init__ / forward              empanada/models/encoders/regnet.py:59-71,88-104
 *          conv_bn_act(groups=...)                    empanada/models/blocks.py:121-171
 * out[p, co] = act(acc * scale[co] + shift[co]), co = grp * group_w + j; acc = sum over the 9 taps and the group's
 * group_w input channels of x[n, oy*stride - 1 + ky, ox*stride - 1 + kx, grp*group_w + c] * w_okkc[co, ky, kx, c],
 * evaluated as ONE fp32 fma chain from +0: taps in raster order; per tap chunks of CK = emp_gconv_chunk(group_w)
 * channels ascending (24, 16 or 8: the largest that divides group_w); per chunk 8-channel slabs j ascending; per
 * slab e = 0, 1; per e the channels 8j + 2kq + e, kq = 0..3 (one v_mfma_f32_16x16x4_f32 = an fmaf chain over its four
 * k's).  Taps outside the image enter as x = 0.  group_w: a multiple of 8 in 8..128; stride 1 or 2.
 * x: base + pixel * x_pixel_stride + channel (0 means groups * group_w), w_okkc: (groups * group_w, 3, 3, group_w) =
 * the Conv2d weight permuted; out likewise with out_pixel_stride.  x, w, out 16-byte aligned, strides % 4 == 0. */
int emp_gconv_chunk(int group_w);
int emp_gconv3x3_bn_act_nhwc(const float *x, int64_t x_pixel_stride, const float *w_okkc, const float *scale,
                             const float *shift, int relu, int N, int H, int W, int groups, int group_w,
                             int stride, float *out, int64_t out_pixel_stride, void *stream);

/* ---- D5: Winograd F(2x2, 3x3) convolution in three calls (3x3, stride 1, padding == dilation) ---------
 * replaces the dilated 3x3 Conv2d -> BatchNorm2d -> ReLU of ASPP and of the dilated ResNet stage
 *          (empanada/models/decoders/aspp.py:22-46, encoders/resnet.py:110-128) where Cin is large.
 * A convolution with dilation d is d*d plain 3x3 convolutions on the sub-grids (y mod d, x mod d); a tile is a
 * 2x2 block of outputs of one sub-grid and reads a 4x4 patch with pixel spacing d.
 * tiles (DEVICE, (T, 3) int32): image index n and (y, x) of the patch's top-left pixel (may be negative: padding);
 *   its outputs are the pixels (y + d + a*d, x + d + b*d), a, b in {0, 1}, that lie inside the image.
 * 1. emp_wino_input_transform: V[p = 4*u + v, t, c] = (B^T patch B)[u, v], B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0;
 *    0 1 0 -1], evaluated as: columns first (t_a0 = d_a0 - d_a2, t_a1 = d_a1 + d_a2, t_a2 = d_a2 - d_a1,
 *    t_a3 = d_a1 - d_a3), then the same combination over rows.  x (N,H,W,C) fp32, V (16, T, C).
 * 2. emp_gemm_nt_batched: C[b] (M, N) = A[b] (M, K) * B[b] (N, K)^T for b < batch, on the fp32 matrix cores with
 *    the fma-chain order of emp_conv_bn_act_nhwc (slabs of S = emp_conv_k_slab(M, N, batch, 0)).  Here M = T, K = Cin, N = Cout,
 *    batch = 16, B = the transformed filters U[p, co, c] = (G g G^T)[u, v] prepared by the host.
 * 3. emp_wino_output_transform: Y = A^T M A per tile, A^T = [1 1 1 0; 0 1 -1 -1], rows first
 *    (s_0 = (m_0 + m_1) + m_2, s_1 = (m_1 - m_2) - m_3), then columns likewise; then the epilogue of
 *    emp_bn_act_nhwc (scale, shift optional) and the scatter to out (N,H,W,Cout), pixel stride out_pixel_stride
 *    (0 means Cout).
 * Alignment.  The transforms move float4: C / Cout % 4 == 0; x, V, Mw, scale, shift and out 16-byte aligned and
 *    out_pixel_stride % 4 == 0 -- unlike emp_conv_bn_act_nhwc there is no scalar store path, so a channel slice that
 *    starts at a channel that is no multiple of 4, or lies in a buffer whose width is none, is refused (EMP_EINVAL,
 *    nothing launched).  The same holds for the output transforms of D5b and D5c.
 *    emp_gemm_nt_batched asks 16 bytes of A and B only (K % 32 == 0): with a C that is not 16-byte aligned, or N % 4
 *    != 0, the tiled kernel stores scalars (such a C is never handed to the weight-stationary or the persistent
 *    kernel); the sums and their order are the same.                                                          */
int emp_wino_input_transform(const float *x, int N, int H, int W, int C, int dil, const int32_t *tiles,
                             int64_t T, float *V, void *stream);
int emp_gemm_nt_batched(const float *A, const float *B, int batch, int64_t M, int N, int K, float *C,
                        void *stream);
/* Steps 1 + 2 in one launch: the GEMM's loader fetches, per tile and position, the four patch pixels B^T d B
 * combines and applies the transform on the way into LDS (same roundings as emp_wino_input_transform), so V is
 * never written.  Mw (16, T, Cout).  N*H*W*Cin < 2^31.                                                       */
int emp_wino_gemm_fused(const float *x, int N, int H, int W, int Cin, int dil, const int32_t *tiles,
                        int64_t T, const float *U, int Cout, float *Mw, void *stream);
int emp_wino_output_transform(const float *Mw, const int32_t *tiles, int64_t T, int N, int H, int W,
                              int Cout, int dil, const float *scale, const float *shift, int relu,
                              float *out, int64_t out_pixel_stride, void *stream);

/* ---- D5b: Winograd F(4x4, 3x3): the same three steps with 6x6 patches, 36 positions, 4x4 outputs per tile ----
 * tiles: (T, 3) int32 (n, y, x) of the patch origin; outputs are (y + d + a*d, x + d + b*d), a, b in 0..3.
 * Input transform  (B^T d B, columns first then rows), per 6-vector d:
 *   r0 = (4 d0 - 5 d2) + d4;  r1 = (d3 + d4) - 4 (d1 + d2);  r2 = (d4 - d3) + 4 (d1 - d2);
 *   r3 = (d4 - d2) + 2 (d3 - d1);  r4 = (d4 - d2) + 2 (d1 - d3);  r5 = (4 d1 - 5 d3) + d5
 * Output transform (A^T m A, rows first then columns), per 6-vector m:
 *   s0 = ((m0 + m1) + m2) + (m3 + m4);  s1 = (m1 - m2) + 2 (m3 - m4);  s2 = (m1 + m2) + 4 (m3 + m4);
 *   s3 = ((m1 - m2) + 8 (m3 - m4)) + m5
 * every operation one fp32 rounding.  V (36, T, C), position p = 6u + v; GEMMs: emp_gemm_nt_batched with batch 36
 * and B = U (36, Cout, Cin) = fp32(G g G^T evaluated in fp64) prepared by the host.  Rounding error is about 10x
 * that of the direct form (1.3e-6 * sum|x||w| measured at K = 18432): stated test tolerance 2e-5 * sum|x||w|.   */
int emp_wino4_input_transform(const float *x, int N, int H, int W, int C, int dil, const int32_t *tiles,
                              int64_t T, float *V, void *stream);
int emp_wino4_output_transform(const float *Mw, const int32_t *tiles, int64_t T, int N, int H, int W,
                               int Cout, int dil, const float *scale, const float *shift, int relu,
                               float *out, int64_t out_pixel_stride, void *stream);
/* D5d: the three steps in ONE launch for 64 -> 64 and 128 -> 128 (emp_wino4.hip): V is kept in LDS one 16-channel slab
 * at a time, M in the accumulators; nothing of V or Mw touches memory, no allocation, no sync.  Same tile table, U and
 * output contract as above; scale AND shift required.  Per M value one fma chain from +0 over 16-channel slabs
 * ascending, inside a slab c, c + 8 for c = 0..7 (a v_mfma_f32_16x16x4_f32 per step j with channels 2j, 2j + 8, 2j + 1,
 * 2j + 9 on k = 0..3): the order of emp_gemm_nt_batched at K-slab 16, so the bits are those of the three calls wherever
 * emp_conv_k_slab(T, Cout, 36, 0) == 16, which the launcher requires (with 16 T Cin < 2^30).
 * emp_wino4_fused_eligible: 1 = _hip.wino4_conv_bn_act takes this kernel (an enabled width pair, both scale and shift,
 * the K-slab 16 plan, at least the measured minimum of tiles; EMP_WINO4_NO_FUSED=1 in the environment turns it off).   */
int emp_wino4_conv_bn_act_nhwc(const float *x, int N, int H, int W, int Cin, int dil, const int32_t *tiles, int64_t T,
                               const float *U, int Cout, const float *scale, const float *shift, int relu,
                               float *out, int64_t out_pixel_stride, void *stream);
int emp_wino4_fused_eligible(int64_t T, int Cin, int Cout, int has_scale_shift);   /* 1 = wino4_conv_bn_act takes the fused kernel */

/* ---- D5c: Winograd F(3x3, 3x3) (points 0, 1, -1, 2, inf): 5x5 patches, 25 positions, 3x3 outputs per tile -----
 * tiles as in D5 with outputs (y + d + a*d, x + d + b*d), a, b in 0..2.  Transforms: r[u] = left fold, over the
 * non-zero entries c of row u in ascending index, of fl(c * d[a]) with fp32 adds (columns first, then rows for
 * the input; rows first, then columns for the output):
 *   B^T = [2 -1 -2 1 0; 0 -2 -1 1 0; 0 2 -3 1 0; 0 -1 0 1 0; 0 2 -1 -2 1],  A^T = [1 1 1 1 0; 0 1 -1 2 0; 0 1 1 4 1].
 * V (25, T, C), p = 5u + v; GEMMs: emp_gemm_nt_batched, batch 25, U (25, Cout, Cin) = fp32(G g G^T in fp64),
 * G = [1/2 0 0; -1/2 -1/2 -1/2; -1/6 1/6 -1/6; 1/6 1/3 2/3; 0 0 1].  Stated tolerance as D5b.                    */
int emp_wino3_input_transform(const float *x, int N, int H, int W, int C, int dil, const int32_t *tiles,
                              int64_t T, float *V, void *stream);
int emp_wino3_output_transform(const float *Mw, const int32_t *tiles, int64_t T, int N, int H, int W,
                               int Cout, int dil, const float *scale, const float *shift, int relu,
                               float *out, int64_t out_pixel_stride, void *stream);

/* ---- D6: 1x1 convolution to 1..4 output channels on NHWC fp32 activations (last layer of every head) ----
 * replaces the final nn.Conv2d(nin, n_classes, 1, bias=True) of PanopticDeepLabHead   empanada/models/heads.py:9-19
 * out[n, co, r] = bias[co] + sum_c x[n*HW + r, c] * w[co, c]; evaluated per wave lane l as an fp32 fma chain from +0
 * over its channel groups (channels 4g..4g+3 of groups g = l, l+64, ...), then a butterfly sum over the 64 lanes
 * (pairs at lane distance 32, 16, 8, 4, 2, 1; each step one fp32 add), then + bias.  x (n_pixels, C) NHWC,
 * w (Cout, C), out planar (N, Cout, pixels_per_image).  C % 4 == 0, C <= 1024, Cout <= 4.                    */
int emp_pointwise_out_nhwc(const float *x, const float *w, const float *bias, int64_t n_pixels,
                           int64_t pixels_per_image, int C, int Cout, float *out, void *stream);

/* ---- D7: BatchNorm(eval) + ReLU + MaxPool2d(3, stride 2, padding 1) on NHWC fp32 (ResNet stem) ------------
 * replaces bn1 -> relu -> maxpool of ResNet.forward             empanada/models/encoders/resnet.py:217-222
 * y[n, oy, ox, c] = max over the 3x3 window (taps outside the image skipped) of max(x*scale[c] + shift[c], 0),
 * multiply and add separate fp32 roundings.  x (N,H,W,C), y (N, (H-1)/2+1, (W-1)/2+1, C), C % 4 == 0.         */
int emp_bn_relu_maxpool_nhwc(const float *x, const float *scale, const float *shift, int N, int H, int W,
                             int C, float *y, void *stream);

/* ---- D9: the whole ResNet stem on a one-channel image: conv 7x7 / 2 + BatchNorm(eval) + ReLU + MaxPool 3x3 / 2 ----
 * replaces conv1 -> bn1 -> relu -> maxpool of ResNet.forward     empanada/models/encoders/resnet.py:186-188,217-222
 * conv[n, oy, ox, co] = ONE fp32 fma chain from +0 over the 49 taps in raster order of x[n, 2oy-3+ky, 2ox-3+kx] *
 * w_tc[7ky+kx, co] (taps outside the image enter as 0; evaluated on the vector ALUs, two channels per v_pk_fma_f32);
 * y = D7 of conv: max over the 3x3 window (outside the image: skipped) of max(conv*scale[co] + shift[co], 0).
 * x (N, H, W) fp32, w_tc (49, 64) = the Conv2d(1, 64, 7) weight as [tap][cout], 16-byte aligned,
 * y (N, PH, PW, 64) NHWC with OH = (H-1)/2+1, PH = (OH-1)/2+1 (likewise W).  The half-resolution activation is never
 * written.                                                                                                        */
int emp_stem_conv7_bn_relu_maxpool(const float *x, const float *w_tc, const float *scale, const float *shift,
                                   int N, int H, int W, float *y, void *stream);

/* ---- D2: logits -> probabilities ---------------------------------------------------------------------------
 * replaces logits_to_prob                                         empanada/inference/engines.py:22-30
 * C == 1: prob = 1 / (1 + expf(-x)) (negation exact, add and divide separate fp32 roundings);
 * C  > 1: softmax over the channel axis: m = max_c x_c, e_c = expf(x_c - m), s = sum of e_c in ascending c from +0,
 *         prob_c = e_c / s.  expf is the device library's (torch's GPU and CPU kernels use their own: results agree within
 *         2 ulp, the hardening decision `p >= thr` on logits within 1e-3 of logit(thr) in all but a few of 2 * 10^6
 *         cases -- tests/test_pipeline_gpu.py).  logits, prob: planar (N, C, HW) fp32; may alias.               */
int emp_logits_to_prob(const float *logits, int N, int C, int64_t HW, float *prob, void *stream);

/* ---- D3 + D2: the x4 up-sampling of a head fused with logits_to_prob ----------------------------------------
 * replaces F.interpolate(scale_factor=4, bilinear, align_corners=True) of a head
 *                                                   empanada/models/panoptic_deeplab.py:100-113
 *          followed by logits_to_prob               empanada/inference/engines.py:22-30
 * x, y, the strides and the bilinear arithmetic as in emp_upsample_bilinear (D3).  prob == 0: y is exactly what
 * emp_upsample_bilinear writes.  prob == 1: y = emp_logits_to_prob (D2) of that value in the same launch -- sigmoid for
 * C == 1, softmax over the C <= 64 channels of a pixel otherwise; the same operations in the same order, so bit-identical
 * to the two calls one after the other, without the full-resolution logits ever being written.  y is typically the
 * [s, e) slice view of a plane's resident head buffer; it must not alias x.                                        */
int emp_upsample_bilinear_prob(const float *x, int N, int C, int h, int w, const int64_t *x_strides,
                               float *y, int H, int W, const int64_t *y_strides, int prob, void *stream);

/* ---- P1 + P2: recursive median over a resident stack, fused with hardening ----------------
 * replaces _MedianQueue.get_next/get_median/end   empanada/inference/engines.py:47-90
 *          _harden_seg / harden_seg               engines.py:114-121, inference/patterns.py:242-251
 * prob  (D, C, HW) fp32 probabilities.  For slice s in [m, D-m) (m = ks/2) the output is the
 * median of {out[s-m..s-1], prob[s..s+m]} (the reference writes the median back into its queue,
 * which makes the filter recursive); the first and last m slices pass through.  Requires
 * D >= ks or ks == 1 (the reference loses slices for shorter stacks; the host mirrors that).
 * out_sem (D, HW) u8: C == 1 -> (p >= thr), C > 1 -> argmax over the filtered channels (first
 * maximum wins); thr is not used for C > 1.  C > 1 keeps C * ks * 1 KiB of filter windows in LDS:
 * above 160 KiB (C * ks > 160) the call fails with EMP_EINVAL.
 * out_prob (D, C, HW) fp32 or NULL: the filtered probabilities.                                */
int emp_median_harden_stack(const float *prob, int D, int C, int64_t HW, int ks, float thr,
                            uint8_t *out_sem, float *out_prob, void *stream);

/* The same filter on a WINDOW of a longer stack, so that the stack never has to be resident at once.
 * prob  (D, C, HW): the window's raw probabilities.
 * hist  (m, C, HW) or NULL: the FILTERED probabilities of the m = ks/2 slices before the window; NULL = the window
 *       starts the axis (its first m slices pass through raw and serve as history, as in emp_median_harden_stack).
 * halo  (m, C, HW) or NULL: the RAW probabilities of the m slices after the window; NULL = the window ends the axis
 *       (its last m slices pass through raw).
 * out_sem  (D, HW) u8, hardened as emp_median_harden_stack does.
 * out_tail (m, C, HW) or NULL: what the filter left for the window's last m slices = the next window's hist.  It may
 *       be the same buffer as hist: a lane reads its history before it writes its tail.
 * With S = hist | prob | halo (absent parts left out), out_sem equals rows [len(hist), len(hist) + D) of the out_sem
 * emp_median_harden_stack(S) writes and out_tail the rows [len(hist) + D - m, len(hist) + D) of its out_prob, bit for
 * bit: cutting a stack into windows and carrying the tail reproduces the whole-stack result.  Nothing is concatenated
 * and no full-size out_prob exists: 4 B read + 1 B written per voxel and channel, plus the m-slice ends.
 * Requires D >= max(m, 1) and, for ks > 1, len(hist) + D + len(halo) >= ks.  ks == 1 hardens only: hist, halo and
 * out_tail must be NULL.  The LDS ceiling of emp_median_harden_stack applies (C > 1: C * ks <= 160).              */
int emp_median_harden_window(const float *hist, const float *prob, const float *halo, int D, int C, int64_t HW,
                             int ks, float thr, uint8_t *out_sem, float *out_tail, void *stream);

/* One streaming step of the same filter: median over ks slices of n floats each.
 * slices_host: host array of ks device pointers; out may alias any of them.
 * replaces _MedianQueue.get_median                 engines.py:59-66                             */
int emp_median_step(const float *const *slices_host, int ks, int64_t n, float *out, void *stream);

/* Harden only (no median): emp_median_harden_stack with ks = 1.  prob (D, C, HW) -> out_sem (D, HW) u8;
 * thr is not used for C > 1.                                                                    */
int emp_harden(const float *prob, int D, int C, int64_t HW, float thr, uint8_t *out_sem,
               void *stream);

/* ---- P3: centre detection ------------------------------------------------------------------
 * replaces find_instance_center                    empanada/inference/postprocess.py:38-76
 * hmp (D, h, w) fp32.  A pixel is a centre when v > thr, v > 0 and v equals the maximum of
 * threshold(v) over the k x k window rows y-k/2 .. y-k/2+k-1 (same for x; -inf padding).
 * out_idx (D, cap) int32 flat indices y*w+x, ascending (raster order) per slice;
 * out_count (D) int32 = number found (may exceed cap: then only `cap` are stored, unordered
 * selection -- the caller must treat count > cap as an error).  cap <= EMP_MAX_CENTERS.
 * thr must be >= 0 (EMP_EINVAL otherwise): the streaming test "v > thr and v > 0" and its
 * comparison of raw neighbours are only proven equal to the reference's for a non-negative
 * threshold, and no configuration uses a negative one.                                          */
int emp_find_centers(const float *hmp, int D, int h, int w, float thr, int k, int cap,
                     int32_t *out_idx, int32_t *out_count, void *stream);

/* The same detection for any capacity 1 <= cap <= EMP_CENTER_LIMIT (no in-LDS sort)
 * replaces find_instance_center                    empanada/inference/postprocess.py:38-76
 * Same rule as emp_find_centers, thr >= 0 included.  The centres of a slice are marked in a bitmap (one bit per pixel)
 * and written out in one ordered pass, so
 *   out_count (D) int32 = exact number found, whatever cap is;
 *   out_idx (D, cap) int32 = the FIRST min(count, cap) centres of each slice in raster order
 *   (deterministic on overflow too; entries past that are left unwritten).
 * work: emp_find_centers_work_elems(D, h, w, cap) int32 elements, 16-byte aligned (zeroed by the call;
 * D * ceil(h*w / 32) rounded up to 4 words per slice; 0 is returned for an invalid shape).          */
int64_t emp_find_centers_work_elems(int D, int h, int w, int cap);
int emp_find_centers_ws(const float *hmp, int D, int h, int w, float thr, int k, int cap, int32_t *work,
                        int32_t *out_idx, int32_t *out_count, void *stream);

/* ---- P4: nearest-centre pixel grouping -----------------------------------------------------
 * replaces group_pixels / chunked_pixel_grouping   postprocess.py:78-169
 * offsets (D, 2, h, w) fp32 (dy, dx) in full-resolution pixel units; step = 1 or 4.
 * id = 1 + index of the first centre with the strictly smallest
 *      d = sqrtf(fmaf(dx, dx, dy*dy)),  dy = step*cy - (step*y + off_y), dx likewise
 * (the rounding torch.norm performs on the reference's CPU path); when K > 20 a pixel whose
 * every d >= 1e5 keeps id 0 (chunked path, :97-111).  K = min(count, cap); K == 0 -> ids 0.
 * 1 <= cap <= EMP_CENTER_LIMIT (ids are uint16: the largest id is 65535); the centres may come in any order.
 * sem (D, h, w) u8 or NULL: when given (same resolution as the offsets), pixels whose class bit is
 * clear in thing_mask are not voted on and get id 0 -- every consumer multiplies the ids by the
 * thing mask anyway (postprocess.py:221, engines.py:280-285), so results downstream are unchanged.
 * work: emp_group_work_elems(D, cap) floats (the centres as fp32 coordinates, read with scalar loads).
 * out_ids (D, h, w) uint16.                                                                     */
int64_t emp_group_work_elems(int D, int cap);
int emp_group_pixels(const int32_t *ctr_idx, const int32_t *ctr_count, int cap,
                     const float *offsets, int D, int h, int w, int step, const uint8_t *sem,
                     uint32_t thing_mask, float *work, uint16_t *out_ids, void *stream);

/* ---- P4b + P5: instance cells -> panoptic labels -------------------------------------------
 * replaces get_instance_cells (nearest upsample)   engines.py:257-275
 *          get_panoptic_seg                        engines.py:277-292, patterns.py:253-277
 *          merge_semantic_and_instance             postprocess.py:223-296
 * sem (D, H, W) u8 class ids (< n_classes <= EMP_MAX_CLASSES); ids (D, H/up, W/up) u16 in 0..cap
 * (nearest-upsampled by `up` on the fly); thing_mask bit c set = class c is a thing.
 * An id above cap counts as 0 (no instance) in every pass, so no id reads or writes past a slice's
 * tables; a class value >= n_classes counts as n_classes - 1.
 * Per instance id (ascending) with >= 1 thing pixel: class = most frequent class among its thing
 * pixels (ties -> smallest), new id = per-class counter from 1, pan = class*div + new id.
 * Non-thing classes: pixels with instance 0 get class*div when their count >= stuff_area.
 * Everything else = void_label.
 * work: int32 workspace of emp_fuse_work_elems(D, cap, n_classes) elements (zeroed by the call).
 * Exactly one of out_pan_u32 / out_pan_i64 (D, H, W) must be non-NULL.                          */
int64_t emp_fuse_work_elems(int D, int cap, int n_classes);
int emp_fuse_panoptic(const uint8_t *sem, const uint16_t *ids, int D, int H, int W, int up,
                      int cap, int n_classes, uint32_t thing_mask, int64_t label_divisor,
                      int64_t stuff_area, int64_t void_label, int32_t *work,
                      uint32_t *out_pan_u32, int64_t *out_pan_i64, void *stream);
/* The two halves of emp_fuse_panoptic, for callers that keep the per-slice tables (and so that each pass can be
 * timed on its own): emp_fuse_lut = histogram + per-slice label table into `work`; emp_fuse_apply = label pass.   */
int emp_fuse_lut(const uint8_t *sem, const uint16_t *ids, int D, int H, int W, int up, int cap,
                 int n_classes, uint32_t thing_mask, int64_t label_divisor, int64_t stuff_area,
                 int32_t *work, void *stream);
int emp_fuse_apply(const uint8_t *sem, const uint16_t *ids, int D, int H, int W, int up, int cap,
                   int n_classes, uint32_t thing_mask, int64_t label_divisor, int64_t void_label,
                   const int32_t *work, uint32_t *out_pan_u32, int64_t *out_pan_i64, void *stream);

/* ---- R1-R3: run extraction + 8-connected components on runs --------------------------------
 * replaces connected_components                    empanada/inference/rle.py:18-24
 *          pan_seg_to_rle_seg                      rle.py:26-86
 *          rle_encode                              empanada/array_utils.py:209-235
 * Step 1  emp_runs_count: row_counts[d*H+y] = number of maximal constant non-zero spans in row y
 *         of slice d of pan (D, H, W) u32.
 * Step 2  emp_exclusive_scan_i32: out[0..n] (n+1 entries) exclusive prefix sum; tmp holds
 *         emp_scan_tmp_elems(n) int32.
 * Step 3  emp_runs_extract: SoA run table in raster order, run i of row r sits at
 *         row_offsets[r] + i: r_start (flat y*W+x0 inside the slice), r_len, r_val.
 * Step 4  emp_runs_label: union-find over runs.  Classes whose bit is set in cc_mask are split
 *         into 8-connected components of equal value and renumbered class*div + k, k = 1.. in
 *         raster order of the component's first pixel, per slice; runs of other classes keep
 *         their value as label (one instance per distinct value).  cc_mask has one bit per class
 *         0..31: a class of 32 or more (value / label_divisor >= 32) is always grouped by value,
 *         whatever the mask, 0xffffffff included.  The Python wrapper (_hip.extract_runs) refuses
 *         a connected-component class outside 0..31 with ValueError rather than group it silently.
 *         k is not limited by label_divisor: the k-th component of a class gets class*div + k even
 *         where k >= div; the class of a component is that of its ORIGINAL value (r_val[c_first]).
 *         Outputs, per run:
 *         r_comp (int32) = dense component index over the whole stack (ordered by first run),
 *         and per component: c_slice, c_label (int64), c_area (int64), c_box (4 x int32:
 *         y0, x0, y1, x1 half-open), c_first (first run).  n_comp_out (device int32[1]).
 *         work: int32 workspace of emp_runs_label_work_elems(n_runs) elements.               */
int emp_runs_count(const uint32_t *pan, int D, int H, int W, int32_t *row_counts, void *stream);
int64_t emp_scan_tmp_elems(int64_t n);
int emp_exclusive_scan_i32(const int32_t *in, int64_t n, int32_t *out, int32_t *tmp, void *stream);
int emp_runs_extract(const uint32_t *pan, int D, int H, int W, const int32_t *row_offsets,
                     int32_t *r_start, int32_t *r_len, uint32_t *r_val, void *stream);
int64_t emp_runs_label_work_elems(int64_t n_runs);
int emp_runs_label(const int32_t *r_start, const int32_t *r_len, const uint32_t *r_val,
                   const int32_t *row_offsets, int64_t n_runs, int D, int H, int W,
                   int64_t label_divisor, uint32_t cc_mask, int32_t *work, int32_t *r_comp,
                   int32_t *c_slice, int64_t *c_label, int64_t *c_area, int32_t *c_box,
                   int32_t *c_first, int32_t *n_comp_out, void *stream);

/* ---- M2: overlaps between components of consecutive slices ---------------------------------
 * replaces rle_intersection / intersection_from_ranges  array_utils.py:340-403 for the pairs the
 *          matcher asks for (rle_matcher                 inference/matcher.py:198-210)
 * For every run of slice d and every run of slice d+1 in the same row whose x-spans overlap and
 * whose values r_val are of the same class (value / label_divisor), appends (comp_a, comp_b, overlap) to out_triplets
 * (cap_triplets x 3 int32, unordered; duplicates of a pair must be summed by the caller).
 * n_out (device int32[1]) counts all triplets found (may exceed the capacity -> error).        */
int emp_runs_overlap_next(const int32_t *r_start, const int32_t *r_len, const int32_t *r_comp,
                          const uint32_t *r_val, const int32_t *row_offsets, int64_t n_runs, int D,
                          int H, int W, int64_t label_divisor, int32_t *out_triplets,
                          int64_t cap_triplets, int32_t *n_out, void *stream);

/* ---- R3: run-length encoding of index lists ----------------------------------------------------
 * replaces rle_encode / rle_decode                empanada/array_utils.py:209-252
 * emp_rle_decode: offsets = exclusive prefix sum of runs (n_runs entries); out_indices receives
 *   starts[i] .. starts[i]+runs[i]-1 at offsets[i].
 * emp_rle_encode: indices (n, ascending) -> maximal runs of consecutive values; out_starts / out_runs hold
 *   up to n entries, n_runs_out (device int32[1]) the count; work: emp_rle_encode_work_elems(n) int32.        */
int emp_rle_decode(const int64_t *starts, const int64_t *runs, const int64_t *offsets, int64_t n_runs,
                   int64_t *out_indices, void *stream);
int64_t emp_rle_encode_work_elems(int64_t n);
int emp_rle_encode(const int64_t *indices, int64_t n, int32_t *work, int64_t *out_starts,
                   int64_t *out_runs, int32_t *n_runs_out, void *stream);

/* ---- M1: box screening ------------------------------------------------------------------------
 * replaces _box_iou / box_iou                     empanada/array_utils.py:144-207 (which pairs exist)
 *          bounding_box_screening                  empanada/consensus.py:197-231
 * boxes (n, 2*ndim) int32, half-open (lo..., hi...); ndim 2 or 3.  Emits every (a, b) whose
 * intersection is strictly positive along every axis; pairs with src_a[a] == src_b[b] are skipped
 * when both src arrays are given; upper_only != 0 keeps only b > a (self-screening without
 * duplicates).  out_pairs (cap, 2) int32 in arbitrary order; n_out (device int32[1]) counts all
 * pairs found (may exceed cap -> caller retries).                                                */
int emp_box_pairs(const int32_t *boxes_a, int64_t na, const int32_t *boxes_b, int64_t nb, int ndim,
                  const int32_t *src_a, const int32_t *src_b, int upper_only, int32_t *out_pairs,
                  int64_t cap, int32_t *n_out, void *stream);

/* ---- M2/C1: intersection of arbitrary RLE pairs --------------------------------------------
 * replaces rle_intersection                        array_utils.py:371-403 (the exact sweep of
 *          intersection_from_ranges :340-369, also for malformed / overlapping runs), as used by
 *          rle_iou :405-429 in object_iou_graph    empanada/consensus.py:276-285
 * Instance i owns runs [inst_off[i], inst_off[i+1]) of (starts, lens) int64; each instance's runs
 * must already be STABLY sorted by start (emp_sort_u64_i32 with key = instance<<40 | start does
 * it).  pairs (n_pairs, 2) int32 instance indices (a, b); out_inter (n_pairs) int64.            */
int emp_rle_pair_intersections(const int64_t *starts, const int64_t *lens, const int64_t *inst_off,
                               const int32_t *pairs, int64_t n_pairs, int64_t *out_inter,
                               void *stream);

/* ---- stable key/value radix sort (rocPRIM via hipCUB), used to order run tables --------------
 * keys 64-bit unsigned, values int32; bits [begin_bit, end_bit) are compared, 0 <= begin_bit <
 * end_bit <= 64; keys that agree in those bits keep their input order, and keys_out holds the whole
 * keys.  Every such range is supported for every n (a range [b, 64) with b > 0 is kept off rocPRIM's
 * merge-sort path, whose comparison mask is wrong for end_bit == 64).
 * work: emp_sort_work_bytes(n) bytes (enough for any bit range); a smaller one is refused.       */
int64_t emp_sort_work_bytes(int64_t n);
int emp_sort_u64_i32(const uint64_t *keys_in, uint64_t *keys_out, const int32_t *vals_in,
                     int32_t *vals_out, int64_t n, int begin_bit, int end_bit, void *work,
                     int64_t work_bytes, void *stream);

/* ---- C3: range voting / joining -------------------------------------------------------------
 * replaces vote_by_ranges / rle_voting / split_range_by_votes / extend_range / join_ranges
 *          empanada/array_utils.py:457-671
 * n ranges [starts[i], ends[i]) int64 (< 2^40), each tagged with a group id grp[i] in
 * [0, n_groups), in any order.  For each group emits, ascending, the maximal ranges covered by
 * at least vote_thr of its input ranges (vote_thr == 1: the union; touching ranges merge -- the
 * reference's sweeps reduce to exactly this coverage count).
 * out_ranges (n, 2) int64 receives all groups back to back; group g owns rows
 * [out_off[g], out_off[g+1]) (out_off: n_groups+1 int32).
 * work: emp_vote_work_bytes(n) bytes.                                                          */
int64_t emp_vote_work_bytes(int64_t n);
int emp_vote_ranges(const int64_t *starts, const int64_t *ends, const int32_t *grp, int64_t n,
                    int n_groups, int vote_thr, void *work, int64_t work_bytes,
                    int64_t *out_ranges, int32_t *out_off, void *stream);

/* ---- R4 / Z1: paint runs into a label volume ------------------------------------------------
 * replaces numpy_fill_instances                    array_utils.py:725-737
 *          fill_func / zarr_fill_instances         empanada/zarr_utils.py:49-58,88-175
 * Runs (starts, lens int64 into the flat volume) carry an order index (position of their
 * instance in dict order) and ids[order] is painted; where runs of different instances overlap
 * the later instance wins, as in the reference's sequential fill.  Runs whose id is 0 are skipped
 * (an instance deleted by a filter neither paints nor shadows).  Runs are cut at 0 and at n_vox.
 * Ids must be < 2^31, and so must every value the volume already holds under a run: voxels are
 * tagged with bit 31 between the two passes, and a value with that bit set would be taken for a
 * tag and index `ids` out of bounds.  The kernel does not check this.  Every Python caller that
 * takes ids or a volume from outside does, on the host, and raises ValueError before any launch
 * (_hip.fill_ids_to_dev, array_utils.numpy_fill_instances, ConsensusResult.paint).  Voxels outside
 * the runs are left as they are.                                                                  */
int emp_fill_runs_u32(uint32_t *vol, int64_t n_vox, const int64_t *starts, const int64_t *lens,
                      const int32_t *order, int64_t n_runs, const uint32_t *ids, void *stream);
int emp_fill_runs_u8(uint8_t *vol, int64_t n_vox, const int64_t *starts, const int64_t *lens,
                     int64_t n_runs, uint8_t value, void *stream);
/* Fill a slab (n_slices, HW) of an xy-stack volume straight from the run table of emp_runs_extract /
 * emp_runs_label: run i paints value[r_comp[i]] at slice c_slice[r_comp[i]] - slice0 (runs whose value
 * is 0 or whose slice falls outside the slab are skipped).  Runs of one stack never overlap.
 * replaces update_trackers + numpy_fill_instances for stack mode (scripts/pdl_inference3d.py:190-233). */
int emp_fill_table_u32(uint32_t *vol, int64_t HW, int n_slices, int slice0, const int32_t *r_start,
                       const int32_t *r_len, const int32_t *r_comp, const int32_t *c_slice,
                       const uint32_t *value, int64_t n_runs, void *stream);

/* ---- T1 (yz plane): runs of a yz stack -> dense (Z, Y, X) label volume -----------------------------
 * replaces the per-pixel decode + sort + re-encode of InstanceTracker.update/finish for axis 'yz'
 *          empanada/inference/tracker.py:83-88,110-113
 * The stack has X slices of (Z, Y) pixels; run i covers pixels r_start[i] .. +r_len[i] (flat z*Y+y) of slice
 * c_slice[r_comp[i]]; voxel (z, y, slice) receives value[r_comp[i]] (0 = skip).  vol must be zeroed.
 * The 3D run-length encoding along x is then obtained with emp_runs_count / emp_runs_extract on vol.   */
int emp_scatter_yz_u32(uint32_t *vol, int Z, int Y, int X, const int32_t *r_start, const int32_t *r_len,
                       const int32_t *r_comp, const int32_t *c_slice, const uint32_t *value,
                       int64_t n_runs, void *stream);

/* ---- M2 (cont.): one triplet per COMPONENT pair -------------------------------------------------------------
 * emp_runs_overlap_next emits one (comp_a, comp_b, pixels) triplet per overlapping run pair; the matcher needs the
 * intersection of two instances (rle_intersection, array_utils.py:371-403), i.e. the sum over all run pairs of the two
 * components.  emp_triplets_reduce sorts the triplets by (a, b) and sums equal pairs on the device: `out` (<= n
 * triplets, ascending (a, b)), n_out device int32.  work: emp_triplets_reduce_work_bytes(n) bytes.               */
int64_t emp_triplets_reduce_work_bytes(int64_t n);
int emp_triplets_reduce(const int32_t *triplets, int64_t n, void *work, int64_t work_bytes, int32_t *out,
                        int32_t *n_out, void *stream);

/* ---- E1: sparse overlap table of two label volumes (ground truth against prediction) --------------------------
 * replaces the instance IoU matrix of Evaluator.__call__   empanada/evaluation/evaluator.py:88-89
 *          rle_matcher                                      empanada/inference/matcher.py:136-232
 *          as input of panoptic_quality                     empanada/evaluation/panoptic_metrics.py:3-54
 *          and of the scores scripts/evaluate3d.py:204-218 prints
 * gt and pred are label arrays of equal shape (R, W), W contiguous; each is uint8 (gt_bytes / pred_bytes = 1) or
 * uint32 (4), read as they are.  The result is every distinct pair (g, p) != (0, 0) that occurs with its voxel count,
 * ascending by (g, p) as unsigned numbers; pairs with one side 0 are included, so the area of a label is a row or
 * column sum.  Counts are integer sums: exact, and the same from run to run.
 * Step 1  emp_label_overlaps_count: row_offsets[0..R] (R+1 int32) = exclusive prefix sum of the number of maximal
 *         spans of constant pair != (0, 0) per row; row_offsets[R] is the span total n_spans, which sizes step 2
 *         exactly.  work: emp_label_overlaps_count_work_bytes(R) bytes.
 * Step 2  emp_label_overlaps: spans -> (key = g << 32 | p, length) -> sort -> sum of equal keys.  out_pairs
 *         (n_spans, 2) int64 and out_counts (n_spans) int64 receive n_out (device int32[1]) rows; the labels must not
 *         have changed since step 1.  work: emp_label_overlaps_work_bytes(n_spans) bytes.
 * A call covers at most 2^31 - 1 voxels (R * W; one span per voxel is the worst case and the scan is int32): a larger
 * array is refused with EMP_EINVAL, never truncated -- callers split the rows into blocks and add the tables
 * (_hip.label_overlaps does).  Per voxel each step reads gt_bytes + pred_bytes bytes; all else is O(n_spans).      */
int64_t emp_label_overlaps_count_work_bytes(int64_t R);
int emp_label_overlaps_count(const void *gt, int gt_bytes, const void *pred, int pred_bytes, int64_t R, int64_t W,
                             void *work, int64_t work_bytes, int32_t *row_offsets, void *stream);
int64_t emp_label_overlaps_work_bytes(int64_t n_spans);
int emp_label_overlaps(const void *gt, int gt_bytes, const void *pred, int pred_bytes, int64_t R, int64_t W,
                       const int32_t *row_offsets, int64_t n_spans, void *work, int64_t work_bytes,
                       int64_t *out_pairs, int64_t *out_counts, int32_t *n_out, void *stream);

/* ---- Z1: zlib streams of label slices, made on the device ----------------------------------------------------
 * replaces zarr's default compressor behind zarr_store.create_dataset(...)   scripts/pdl_inference3d.py:228-233
 *          (the reference stores its label volumes compressed, on the CPU)
 * src is a slab of n_chunks slices of chunk_bytes = Y * X * item bytes each, C order, little endian, item = 1 (uint8)
 * or 4 (uint32).  Every slice becomes one zlib stream (RFC 1950 / 1951) that any inflate decodes:
 *     78 01 | seg_0 | seg_1 | ... | seg_{S-1} | 03 00 | adler32(raw), 4 bytes big-endian
 * seg_k covers raw bytes [k * SEG, min(chunk_bytes, (k + 1) * SEG)), SEG = 4096.  Each segment is one fixed-Huffman
 * block -- header bits 0,1,0 (BFINAL = 0, BTYPE = 01), the tokens, end-of-block (symbol 256) -- followed by an empty
 * stored block: bits 0,0,0, zero bits up to the byte boundary, 00 00 FF FF.  So every segment ends byte-aligned and
 * segments, and chunks, are concatenated as bytes.  03 00 is the empty final fixed block.
 * Tokens, in element order: an element equal to the element before it in the chunk (also across a segment border,
 * never across chunks: a chunk's first element is literal) is part of a repeat.  A maximal repeat of n bytes inside
 * the segment is written as matches at distance `item` (distance code 0 or 3, five bits, no extra bits): length-258
 * matches while n >= 261 or n == 258, then n = 259 / 260 as (n - 3, 3), then one match for 3 <= n <= 258; 1 or 2
 * bytes (item 1 only) as literals.  Any other element is `item` literal bytes, 8 bits for values below 144 and 9
 * for the rest.  Huffman codes are packed most significant bit first, extra bits least significant first.
 * Worst case per chunk: emp_deflate_bound = 2 + ceil(9 L / 8) + 8 ceil(L / SEG) + 6 bytes, L = chunk_bytes.
 * Step 1  emp_deflate_count: offsets[0..n_chunks] (device int64) = byte offset of every chunk's stream in the output;
 *         offsets[n_chunks] is the total, which sizes step 2 exactly.  It also leaves the segment offsets and the
 *         chunks' Adler-32 in `work` (emp_deflate_work_bytes bytes), which step 2 reads.
 * Step 2  emp_deflate_encode: the streams, to out[0, total); nothing outside is written.  src and work must not have
 *         changed since step 1 -- a segment whose size is no longer the counted one is left out, never overrun.
 * A call's worst case (n_chunks * bound) must stay within 2^31 - 1 bytes (the segment sizes are scanned in int32): a
 * larger slab is refused with EMP_EINVAL, callers split it into blocks of chunks (_hip.deflate_labels does).
 * Per raw byte each step reads one byte; step 2 writes the compressed bytes; all else is per segment.
 * The bound and the workspace query return -1 (and set emp_last_error) for arguments the steps would refuse.       */
int64_t emp_deflate_bound(int64_t chunk_bytes, int item);
int64_t emp_deflate_work_bytes(int64_t n_chunks, int64_t chunk_bytes, int item);
int emp_deflate_count(const void *src, int item, int64_t n_chunks, int64_t chunk_bytes, void *work,
                      int64_t work_bytes, int64_t *offsets, void *stream);
int emp_deflate_encode(const void *src, int item, int64_t n_chunks, int64_t chunk_bytes, void *work,
                       int64_t work_bytes, int64_t total, uint8_t *out, int64_t out_bytes, void *stream);

/* ---- Z2: one level of a multiscale label pyramid: mode pooling on the device -------------------------------------
 * no counterpart in the reference: its label volumes are written at full resolution only (scripts/pdl_inference3d.py:
 * 225-233) and viewers (napari, neuroglancer, every OME-NGFF reader) down-sample them on the CPU after the fact.
 * src is a contiguous (D, H, W) array of item-byte unsigned little-endian integers, item = 1 (uint8) or 4 (uint32);
 * fz, fy, fx are each 1 or 2, at least one of them 2; dst is a contiguous (ceil(D / fz), ceil(H / fy), ceil(W / fx))
 * array of the same item size that does not overlap src.
 * dst[z, y, x] = the value that occurs most often among the src voxels of the cell [fz z, fz z + fz) x [fy y, fy y +
 * fy) x [fx x, fx x + fx) clipped to the volume (at odd sizes the last cells hold 4, 2 or 1 voxels); among values that
 * occur equally often the LARGEST wins, compared as unsigned numbers.  So background 0 never wins a tie, a sheet one
 * voxel thick survives a 4 : 4 split, and the result does not depend on any visiting order.
 * One streaming pass: reads fz fy fx elements and writes one per output voxel, 16-byte loads and stores where the
 * rows of src (W * item) and of dst start on 16-byte addresses, element-wise ones with the same results otherwise;
 * all index arithmetic is 64-bit.  No workspace, no allocation, no synchronisation; an empty volume is a no-op.  */
int emp_label_pool_mode(const void *src, int item, int64_t D, int64_t H, int64_t W, int fz, int fy, int fx, void *dst,
                        void *stream);

/* ---- E2: per-object measurements of a label volume (voxels, box, index sums, exposed faces) ------------------------
 * no counterpart in the reference: its trackers carry boxes and runs per plane, before the consensus
 * (empanada/inference/tracker.py:61-123); the morphology of the final objects is left to CPU code run afterwards.
 * lab is a contiguous (D, H, W) array of item-byte unsigned little-endian integers, item = 1 (uint8) or 4 (uint32; the
 * bits of an int32 are taken as they are), 0 = background.  The table has one row of 14 int64 per distinct non-zero
 * label, ascending by label as an unsigned number:
 *     0        label
 *     1        voxels
 *     2..4     z0, y0, x0   smallest index per axis, z counted as z_base + local z
 *     5..7     z1, y1, x1   largest index + 1
 *     8..10    sum_z, sum_y, sum_x   sums of the voxel indices (z including z_base)
 *     11..13   faces_z, faces_y, faces_x   exposed voxel faces normal to each axis
 * A face of a voxel is exposed when the voxel on its other side carries a different value; background counts as
 * different and a position outside the array reads as 0.  Along z the block has two optional neighbour slices, `below`
 * (z = -1) and `above` (z = D), each a contiguous (H, W) array of the same item size, which stand in for what lies
 * outside the block; a null pointer means 0.  Columns 1 and 8..13 are sums and 2..7 minima / maxima of integers, so the
 * table of a volume equals the merge (sum, min, max per label) of the tables of any z-partition of it whose blocks
 * were given their true neighbour slices, and no visiting order shows in the result.  The face count is the "crack"
 * area: exact and additive, but it overestimates a smooth surface (1.5 x for a sphere).
 * Step 1  emp_label_measure_count: row_offsets[0..R] (R + 1 int32, R = D * H) = exclusive prefix sum of the number of
 *         maximal runs of one non-zero label per row; row_offsets[R] is the run total n_runs, which sizes step 2
 *         exactly.  work: emp_label_measure_count_work_bytes(R) bytes.
 * Step 2  emp_label_measure: runs -> (label, row, x start, length, y exposure, z exposure) -> sort by label -> one row
 *         per label.  out_table (n_runs, 14) int64 receives n_out (device int32[1]) rows; the labels must not have
 *         changed since step 1 (a run past n_runs is dropped, never written).  work: emp_label_measure_work_bytes(
 *         n_runs) bytes.
 * A call covers at most 2^31 - 1 voxels (D * H * W; one run per voxel is the worst case and the scan is int32): a
 * larger block is refused with EMP_EINVAL, never truncated -- callers cut the slab into z-blocks, hand each its
 * neighbour slices and merge the tables (_hip.measure_labels does).  Step 1 reads every voxel once; step 2 reads every
 * voxel once and, for the lanes that hold a non-zero voxel, the same positions of rows y +- 1 and z +- 1; all else is
 * O(n_runs).                                                                                                        */
int64_t emp_label_measure_count_work_bytes(int64_t R);
int emp_label_measure_count(const void *lab, int item, int64_t D, int64_t H, int64_t W, void *work, int64_t work_bytes,
                            int32_t *row_offsets, void *stream);
int64_t emp_label_measure_work_bytes(int64_t n_runs);
int emp_label_measure(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, const void *above,
                      int64_t z_base, const int32_t *row_offsets, int64_t n_runs, void *work, int64_t work_bytes,
                      int64_t *out_table, int32_t *n_out, void *stream);

/* ---- E3: 3D connected components of a label volume, and painting a value per component ------------------------------
 * replaces, on the device, what users of the reference run on a CPU after the fact: cc3d.connected_components (the
 *          multi-label rule) and cc3d.dust; the reference itself never checks that an instance is one piece.
 * lab is a contiguous (D, H, W) array of item-byte unsigned little-endian integers, item = 1 (uint8) or 4 (uint32; the
 * bits of an int32 are taken as they are), 0 = background.  connectivity is 6, 18 or 26: two voxels are neighbours when
 * their indices differ by at most 1 on every axis and on exactly one axis (6), at most two (18), any number (26).  Two
 * voxels belong to one component when they carry the same non-zero value and a chain of neighbours of that value joins
 * them; voxels of different values never join.  Components are numbered k = 0 .. n - 1 ascending by the flat index
 * (z H + y) W + x of their first voxel in raster order.  The table has one row of 9 int64 per component, in that order:
 *     0        label (the value)
 *     1        voxels
 *     2        first: flat index of the first voxel, with z_base H W added
 *     3..5     z0, y0, x0   smallest index per axis, z counted as z_base + local z
 *     6..8     z1, y1, x1   largest index + 1
 * Sets are joined by integer atomicMin on run indices and the columns are integer sums, minima and maxima, so no
 * visiting order, atomic order or launch shape shows in any output.
 * Step 1  emp_label_measure_count (E2): the run count of E3 is E2's -- maximal runs of one non-zero label per row.
 * Step 2  emp_label_components: runs -> (row, x start, x end, label) -> union-find over the runs -> roots numbered by
 *         first run -> voxels and boxes per component.  A run searches the rows (z, y - 1) and (z - 1, y), and for 18 /
 *         26 also (z - 1, y - 1) and (z - 1, y + 1), for runs of its own label whose x range overlaps its own; the
 *         range is widened by one voxel on either side where the connectivity allows the step along x on top: for the
 *         first two rows from 18 on, for the last two for 26 alone.  out_table (n_runs, 9) int64 receives n_out (device
 *         int32[1]) rows; the runs and their component index stay in `work` (emp_label_components_work_bytes(n_runs)
 *         bytes) for step 3.  The labels must not have changed since step 1.
 * Step 3  emp_label_components_paint: dst, a contiguous (z_hi - z_lo, H, W) array of dst_item (1 or 4) bytes per voxel,
 *         receives lut[component] (uint32, n_comp entries, 0 = erase) over every run's voxels of slices [z_lo, z_hi).
 *         If dst is those slices of lab themselves (same address, same item size) only run voxels are written, and only
 *         those of runs whose value changes; any other dst must not overlap lab and has its background written as 0.
 *         lab, row_offsets, n_runs and work are those of step 2; lab is not read.  The low dst_item bytes of a value are
 *         written: the caller refuses a lut with a value above 255 for dst_item 1 before the call (_hip does, and
 *         nothing is written).  16-byte stores where a run covers a whole 16-byte group, element stores at its ends.
 * A call covers at most 2^31 - 1 voxels (D * H * W), as for E1 / E2: a larger block is refused with EMP_EINVAL --
 * callers cut the slab into z-blocks, label each by itself and join the blocks' components across the seams on the
 * host (_hip.label_components, components.merge_blocks).  Step 2 reads every voxel once; step 3 writes the voxels of
 * the runs it paints (and the background once where dst is not lab); all else is O(n_runs), all index arithmetic 64-bit. */
int64_t emp_label_components_work_bytes(int64_t n_runs);
int emp_label_components(const void *lab, int item, int64_t D, int64_t H, int64_t W, int connectivity, int64_t z_base,
                         const int32_t *row_offsets, int64_t n_runs, void *work, int64_t work_bytes, int64_t *out_table,
                         int32_t *n_out, void *stream);
int emp_label_components_paint(const void *lab, int item, int64_t D, int64_t H, int64_t W, const int32_t *row_offsets,
                               int64_t n_runs, const void *work, int64_t work_bytes, const uint32_t *lut, int64_t n_comp,
                               int64_t z_lo, int64_t z_hi, void *dst, int dst_item, void *stream);

/* ---- E4: background cavities of a label volume, for filling the holes enclosed in objects ---------------------------
 * replaces, on the device, what users of the reference run on a CPU after the fact: scipy.ndimage.binary_fill_holes or
 *          fill_voids object by object (the napari front-end's "fill holes in segmentation" switch).
 * lab is a contiguous (D, H, W) array of item-byte unsigned little-endian integers, item = 1 (uint8) or 4 (uint32; the
 * bits of an int32 are taken as they are), 0 = background.
 *   - A cavity is a 6-connected component of the zero voxels (indices differ by 1 on exactly one axis): the complement
 *     of 26-connected objects, so a diagonal leak does not open a cavity.
 *   - A cavity is open if one of its voxels lies on the border of the WHOLE volume (index 0 or size - 1 on any axis),
 *     closed otherwise.
 *   - The wall labels of a cavity are the non-zero values of the voxels that share a FACE with one of its voxels; a
 *     voxel that touches it only across an edge or a corner does not count.  Labels compare as unsigned 32-bit numbers.
 *   - A closed cavity is filled with L if and only if its wall labels are exactly {L} (lab_min == lab_max == L) and,
 *     with a cap max_voxels, voxels <= max_voxels.  A closed cavity walled by two or more labels -- a gap between
 *     touching objects, the shell around an object nested in another -- is left alone and counted as shared.
 * Cavities are numbered k = 0 .. n - 1 ascending by the flat index (z H + y) W + x of their first voxel in raster
 * order.  The table has one row of 10 int64 per cavity, in that order:
 *     0        voxels
 *     1        first: flat index of the first voxel, with z_base H W added
 *     2..4     z0, y0, x0   smallest index per axis, z counted as z_base + local z
 *     5..7     z1, y1, x1   largest index + 1
 *     8        lab_min: smallest wall label, 2^32 if none was surveyed
 *     9        lab_max: largest wall label, 0 if none was surveyed
 * Openness is no column: the host derives it from the box against the whole volume's shape (holes.plan), after the
 * tables of z-blocks and ranks have been merged, so neither needs a special case.  A component whose box touches x = 0,
 * x = W, y = 0 or y = H of the block is open whatever lies beyond the block in z: its wall is NOT surveyed and it
 * reports (2^32, 0).  Every other component is bounded by non-zero voxels along x, so its lab_max is non-zero: lab_max
 * == 0 is the mark "touches an x or y border", and a merge of block tables gives (2^32, 0) to every merged component
 * that has a piece with that mark (holes.merge_blocks), which is what the undivided volume reports.  The outside
 * background is one such component and holds most zero runs of a volume, so the survey costs in proportion to the
 * voxels of candidate cavities, not of the volume.  Along z the block has two optional neighbour slices as in E2,
 * `below` (z = -1) and `above` (z = D): a null pointer means "no neighbour there", and the labels of a neighbour slice
 * over a cavity's voxels enter its wall labels (zero voxels there are the business of the seam: components.seam_pairs).
 * Sets are joined by integer atomicMin on run indices and the columns are integer sums, minima and maxima, so no
 * visiting order, atomic order, launch shape or z-partition shows in any output.
 * Step 1  emp_label_holes_count: row_offsets[0..R] (R + 1 int32, R = D * H) = exclusive prefix sum of the number of
 *         maximal runs of ZERO voxels per row; row_offsets[R] is the run total n_runs.  work:
 *         emp_label_holes_count_work_bytes(R) bytes.
 * Step 2  emp_label_holes: zero runs -> (row, x start, x end, 0) -> E3's union-find with connectivity 6 (rows (z, y - 1)
 *         and (z - 1, y), x ranges overlapping, not widened) -> roots numbered by first run -> voxels and boxes, reduced
 *         over the wave before one atomic per segment of equal component (the outside component alone holds millions
 *         of runs) -> wall labels of the candidates: the voxels just before and after a run along x, and the voxels over
 *         the run's x range in rows y +- 1 and z +- 1.  out_table (n_runs, 10) int64 receives n_out (device int32[1])
 *         rows; the runs and their component index stay in `work` (emp_label_holes_work_bytes(n_runs) bytes) in E3's
 *         layout.  The labels must not have changed since step 1.
 * Step 3  emp_label_components_paint (E3) with lab, row_offsets, n_runs and work of step 2 and dst = the slices [z_lo,
 *         z_hi) of lab themselves: every run's value is 0, so in place it writes lut[component] over the runs whose lut
 *         entry is non-zero and nothing else -- nothing but voxels of filled cavities is written.
 * A call covers at most 2^31 - 1 voxels (D * H * W), as for E2 / E3: a larger block is refused with EMP_EINVAL --
 * callers cut the slab into z-blocks, hand each its neighbour slices and join the blocks' components across the seams
 * on the host (_hip.label_holes, holes.merge_blocks).  Step 1 and step 2 read every voxel once (16-byte loads of uint32
 * and 4-byte loads of uint8 per lane where the group lies on such an address, element-wise loads with the same results
 * otherwise); the survey reads, element-wise, six neighbours' worth of the candidates' voxels; all else is O(n_runs),
 * all index arithmetic 64-bit.  No memset node: counts and workspace are zeroed by kernels, so every step can be
 * captured.  An empty slab and n_runs == 0 (no zero voxel) are no-ops with n_out = 0.                                 */
int64_t emp_label_holes_count_work_bytes(int64_t R);
int emp_label_holes_count(const void *lab, int item, int64_t D, int64_t H, int64_t W, void *work, int64_t work_bytes,
                          int32_t *row_offsets, void *stream);
int64_t emp_label_holes_work_bytes(int64_t n_runs);
int emp_label_holes(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, const void *above,
                    int64_t z_base, const int32_t *row_offsets, int64_t n_runs, void *work, int64_t work_bytes,
                    int64_t *out_table, int32_t *n_out, void *stream);

/* ---- E5: label morphology -- exact Euclidean erode and dilate of a label volume, and the distance under both ---------
 * replaces, on the device, what users of the reference run on a CPU after the fact: scipy.ndimage.binary_erosion /
 *          binary_dilation / binary_opening / binary_closing or an edt per object (the napari front-end's label tools).
 * lab is a contiguous (D, H, W) array of item-byte unsigned little-endian integers, item = 1 (uint8) or 4 (uint32; the
 * bits of an int32 are taken as they are), 0 = background.  Every 32-bit value is a legal label: there is no sentinel.
 * The sampling (az, ay, ax), integers in 1 .. 16, is the voxel pitch per axis, and the squared distance of two voxels is
 * d2(v, u) = (az dz)^2 + (ay dy)^2 + (ax dx)^2, an exact integer.
 *   - Inside distance: for lab[v] != 0, edt(v) = min(cap, min over the voxels u of the volume with lab[u] != lab[v] of
 *     d2(v, u)) -- background and other objects count alike; positions outside the volume are no candidates (as in
 *     scipy.ndimage.distance_transform_edt: an object cut by the volume's face is not eroded from that face); without a
 *     candidate the value is cap.  For lab[v] == 0 the value is 0.  1 <= cap <= 65535, so a uint16 holds every value.
 *   - Nearest label: for lab[v] == 0, among the voxels u with lab[u] != 0 and d2(v, u) <= r2 the one with the smallest
 *     d2, among equal d2 the largest label under unsigned comparison (the pooling kernel's tie rule); 0 if there is none.
 *   - erode:  lab[v] where edt(v) > r2 (computed with cap = r2 + 1), 0 elsewhere: touching objects get a gap.
 *   - dilate: lab[v] where it is non-zero -- an object never overwrites another -- and the nearest label elsewhere.
 *   1 <= r2 <= 65534 and r2 >= min(az, ay, ax)^2: below that the ball is a point and the call is refused.
 * The volume may be continued along z by two halo stacks as E2's neighbour slices are, but of any depth: `below` holds
 * hb >= 0 slices that stand for z = -hb .. -1 and `above` ha >= 0 slices for z = D .. D + ha - 1; a count of 0 means the
 * volume's face.  Halo voxels are candidates like any other; the output covers the D slices of lab alone.  With
 * floor(sqrt(r2)) / az slices on either side (floor(sqrt(cap - 1)) / az for the distance) the result is that of the
 * undivided volume, so z-blocks and the ranks' slabs need no merge.
 * Both are computed separably, x then y then z, with w = a_axis^2.  Distance: f = cap on non-zero voxels; in each pass,
 * for voxel p of label l, best = f[p] and on either side, for k = 1, 2, ... while w k^2 < best: leaving the volume
 * stops the side; lab[q] != l takes w k^2 and stops the side (that voxel is itself a candidate and all beyond it are
 * farther); otherwise best = min(best, f[q] + w k^2).  Nearest label: the passes carry the key (d2, label), starting as
 * (0, lab) on labelled voxels and (r2 + 1, 0) elsewhere, with no stop at labels and k running while w k^2 <= min(best
 * d2, r2) so that ties are seen.  All arithmetic is integer, there is no atomic and no kernel waits for another, so no
 * launch shape or z-partition shows in any output.
 * out is never lab: a pass reads its neighbours' labels.  The intermediates live in `work`, which kernels initialise (no
 * memset node): two uint16 per voxel of the extended volume for emp_label_edt / emp_label_erode
 * (emp_label_edt_work_bytes), two uint16 and two uint32 for emp_label_dilate (emp_label_dilate_work_bytes); the queries
 * return -1 for a shape that a call would refuse.  A call covers at most 2^31 - 1 voxels, halos included: a larger
 * block is refused with EMP_EINVAL, as is every other argument error, before any launch.  D == 0 is a no-op.
 * emp_label_edt writes the (D, H, W) uint16 distances, emp_label_erode and emp_label_dilate a (D, H, W) label volume of
 * the same item size.                                                                                                */
int64_t emp_label_edt_work_bytes(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha);
int emp_label_edt(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, int64_t hb,
                  const void *above, int64_t ha, int az, int ay, int ax, int cap, void *work, int64_t work_bytes,
                  uint16_t *out, void *stream);
int emp_label_erode(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, int64_t hb,
                    const void *above, int64_t ha, int az, int ay, int ax, int r2, void *work, int64_t work_bytes,
                    void *out, void *stream);
int64_t emp_label_dilate_work_bytes(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha);
int emp_label_dilate(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, int64_t hb,
                     const void *above, int64_t ha, int az, int ay, int ax, int r2, void *work, int64_t work_bytes,
                     void *out, void *stream);

/* ---- E6: geodesic growth -- seeds regrown inside the objects of a label volume -----------------------------------------
 * replaces, on the device, the flood that users of the reference run on a CPU to separate touching objects: erode, label
 *          the cores, grow them back inside the object (a watershed on a binary mask).
 * Inputs.  L: a label volume (D, H, W), item = 1 (uint8) or 4 (uint32; the bits of an int32 are taken as they are); every
 * 32-bit value other than 0 is a label.  S: a seed volume, uint32, of the same shape; a seed on a voxel with L = 0 is
 * ignored.
 * Geodesic distance.  For a voxel v with L(v) = l != 0, g(v) is the number of steps of the shortest 6-connected path
 * from v to a seed voxel, where EVERY voxel of the path carries the label l.  If no such path exists, g(v) = infinity.
 * Seeds have g = 0.  The distance is a 32-bit count and has no cap.
 * Owner.   g(v) = 0:               owner(v) = S(v)
 *          g(v) = k >= 1, finite:  the largest owner(u), compared unsigned, over the face neighbours u of v with
 *                                  L(u) = l and g(u) = k - 1
 *          g(v) = infinity or L(v) = 0:  owner(v) = 0
 *   - The tie rule is the one the pooling and dilation kernels use.
 *   - Induction over k makes the owner unique.
 *   - Growth never crosses from one label into another and never enters background.
 *   - Positions outside the volume are no neighbours.
 * Equivalent fixed point.  It is what makes a parallel schedule legal.
 *   - Keep one key per voxel: dist << 32 | ~owner.
 *   - Seeds are fixed at 0 << 32 | ~S.
 *   - Every other labelled voxel repeatedly takes min over same-label face neighbours of (key(u) + (1 << 32)).
 *   - All-ones means "not reached" (and stays all-ones under the addition).
 *   - Started from all-ones, the keys only fall.
 *   - The unique fixed point is the definition above, in whatever order voxels are updated.
 * Relation to the reference.  Its inference/watershed.py:mask_watershed is a FIFO flood from the markers with
 * connectivity 1.  It computes the same distances and differs only in who wins a tie: there the first in queue order,
 * here the largest owner.  No BC engine is part of this.
 * `state` is the (D, H, W) array of those keys, one aligned uint64 per voxel, owned by the caller: it is the interface
 * between sweeps, z-blocks and ranks.  `work` (emp_label_grow_work_bytes; -1 for a shape that a call would refuse) holds
 * the list of tiles (8 x 8 x 64 voxels) that hold a labelled voxel, two byte arrays of the tiles that are due, and the
 * counters; kernels initialise all of it.  A call covers at most 2^31 - 1 voxels: a larger one is refused with
 * EMP_EINVAL, as is every other argument error, before any launch.  D == 0 is a no-op.
 * emp_label_grow_init   writes every key (seeds 0 << 32 | ~S, all else all-ones), the list, and marks as due the tiles
 *                       that hold a seed or face one.  work + 0 then holds the uint64 length of the list.
 * emp_label_grow_sweep  one workgroup per listed tile (n_listed = that length); a tile that is not due is left at once.
 *                       The others load the tile and a one-voxel ring of labels and keys into LDS, relax there until
 *                       nothing in the tile changes, write the lowered keys back and mark the tiles behind the faces
 *                       on which a key fell as due for the next sweep.  The ring reads the keys as they are at that
 *                       moment.  below / above: ONE slice each of (labels, state) of the neighbouring z-block or rank,
 *                       both null = the volume's face; force bit 0 / 1 runs the tiles on the first / last slice
 *                       whatever their marks say (the halo has changed).  turn: 0 for the first sweep after the
 *                       initialisation, then alternating -- which of the two mark arrays is read.  A block that stored
 *                       anything adds one to the uint64 at work + 8 (1 + slot), slot in 0 .. 7: a sweep after which
 *                       its counter has not moved has reached the fixed point of what it could see.
 * emp_label_grow_paint  over n voxels: mode 0, dst = owner ? lut[owner] : L (lut: n_lut uint32, entry 0 unused; an owner
 *                       >= n_lut keeps L), in place on the labels -- only voxels whose value changes are written -- or
 *                       into another array of item size 1 or 4 that does not overlap them; mode 1, dst = owner, uint32. */
int64_t emp_label_grow_work_bytes(int64_t D, int64_t H, int64_t W);
int emp_label_grow_init(const void *lab, int item, const uint32_t *seeds, int64_t D, int64_t H, int64_t W,
                        uint64_t *state, void *work, int64_t work_bytes, void *stream);
int emp_label_grow_sweep(const void *lab, int item, int64_t D, int64_t H, int64_t W, uint64_t *state,
                         const void *below_lab, const uint64_t *below_state, const void *above_lab,
                         const uint64_t *above_state, void *work, int64_t work_bytes, int64_t n_listed, int turn,
                         int force, int slot, void *stream);
int emp_label_grow_paint(const uint64_t *state, const void *lab, int item, int64_t n, const uint32_t *lut,
                         int64_t n_lut, int mode, void *dst, int dst_item, void *stream);

/* ---- E7: surface meshes of a label volume (welded, outward-oriented quads of the exposed voxel faces) ---------------
 * replaces, on the device, what users of the reference run on a CPU after the fact, object by object:
 *          skimage.measure.marching_cubes or zmesh over a volume that was already resident.
 * lab is a contiguous (D, H, W) array as in E2 (item = 1 or 4, 0 = background), with E2's optional neighbour slices
 * `below` (z = -1) and `above` (z = D); a position outside the array reads as 0.
 * Lattice.  Voxel (z, y, x) occupies [z, z + 1] x [y, y + 1] x [x, x + 1].  A corner is an integer point (z, y, x) with
 *   0 <= z <= depth, 0 <= y <= H, 0 <= x <= W, and its number is (z_base + z) (H + 1) (W + 1) + y (W + 1) + x.
 * Faces.  Label L != 0 owns one quad for every face of one of its voxels that E2 calls exposed: the voxel on the other
 *   side has a different value.  A face between two different labels gives two quads, one per label, with opposite
 *   windings.  Per object and axis the number of quads equals columns 11..13 of E2's table.
 * Winding.  Every quad starts at its lowest corner o; with ez, ey, ex the unit steps its corners are, in order,
 *     -z (0)  o, o+ex, o+ey+ex, o+ey        +z (1)  o, o+ey, o+ey+ex, o+ex
 *     -y (2)  o, o+ez, o+ez+ex, o+ex        +y (3)  o, o+ex, o+ex+ez, o+ez
 *     -x (4)  o, o+ey, o+ez+ey, o+ez        +x (5)  o, o+ez, o+ez+ey, o+ey
 *   (the number is the direction code).  The arbiter: with vertices as (z, y, x) triples, the sum over an object's quads
 *   of det[p0, p1, p2] + det[p0, p2, p3] is exactly 6 x the object's voxel count.
 * Vertices.  One per (label, corner) pair that at least one of the label's quads touches; equivalently, of the eight
 *   voxels around the corner at least one is L and at least one is not.  A corner can carry up to eight vertices.  Two
 *   voxels of L that meet only along an edge or at a corner share those vertices, so an edge may carry four quads of
 *   one object; it is not split.
 * Order.  Vertices ascend by (label as unsigned, z, y, x): by the key label << 32 | corner.  Quads ascend by (label,
 *   z, y, x of the owning voxel, direction code).  Both are fixed by the definition: bit-identical from run to run and
 *   from any z-partition whose blocks were given their true neighbour slices.
 * Outputs.  vertices (nv, 3) int32 in zyx order; quads (nq, 4) int32, indices into vertices; objects (n, 5) int64 --
 *   label, v_begin, v_end, q_begin, q_end -- ascending by label, the rows of E2's table.
 * Limits, refused with EMP_EINVAL and never truncated: (depth + 1) (H + 1) (W + 1) <= 2^32 for the whole volume (the
 *   key holds the corner in 32 bits; about 1624^3), nv and nq below 2^31, and D H W <= 2^26 per call of steps 1 and 2
 *   (6 quads and 8 keys per voxel seen at most: the int32 scan stays exact) -- callers cut z-blocks.
 * A block owns the corner planes 0 .. D - 1 and, with `top` (the volume's last block), plane D: a seam plane is emitted
 * once, by the block above it, which sees the same eight voxels through `below`.
 * Step 1  emp_label_mesh_count: R = D H + (D + top) (H + 1) rows -- the voxel rows, then the owned corner rows -- and
 *         row_offsets[0..R] (R + 1 int32) = exclusive prefix sum of the quads per voxel row and the keys per corner
 *         row: row_offsets[D H] is the quad total n_quads, row_offsets[R] - n_quads the key total n_keys.  work:
 *         emp_label_mesh_count_work_bytes(R) bytes.
 * Step 2  emp_label_mesh_emit: vkeys[n_keys] = label << 32 | corner in corner order; per quad qkeys = label << 32 | its
 *         lowest corner o and qdirs = its direction code, in (z, y, x, direction) order.  The labels must not have
 *         changed since step 1 (an item past the totals is dropped, never written).
 * Step 3  the caller sorts vkeys over all 64 bits and (qkeys, qdirs) stably over bits 32..63 (emp_sort_u64_i32); keys
 *         and quads of several blocks or ranks are concatenated in z order first.
 * Step 4  emp_label_mesh_index: sorted keys -> vertices and objects (at most max_objects rows are written; n_objects,
 *         a device int32, receives the number of labels), sorted quads -> quads, each corner found by a binary search
 *         inside its object's [v_begin, v_end); -1 where the keys hold no such vertex.  work:
 *         emp_label_mesh_index_work_bytes(nv) bytes.
 * No step uses atomics and no order depends on scheduling.
 * Smoothing.  Every quad edge joins two lattice neighbours, so a vertex has at most six neighbours, one per direction
 *   code.  emp_mesh_neighbours fills nbr (nv, 6) int32, -1 = none.  emp_mesh_smooth is one step dst = src + factor (m -
 *   src) over (nv, 3) float32, m the mean of the present neighbours added in slot order; src and dst must differ.  One
 *   Taubin iteration is a step with lambda = 0.5 and one with mu = -0.53.  Each object is smoothed by itself: touching
 *   objects may drift apart or overlap by a fraction of a voxel.                                                       */
int64_t emp_label_mesh_count_work_bytes(int64_t R);
int emp_label_mesh_count(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below,
                         const void *above, int top, void *work, int64_t work_bytes, int32_t *row_offsets, void *stream);
int emp_label_mesh_emit(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, const void *above,
                        int top, int64_t z_base, const int32_t *row_offsets, int64_t n_quads, int64_t n_keys,
                        uint64_t *vkeys, uint64_t *qkeys, int32_t *qdirs, void *stream);
int64_t emp_label_mesh_index_work_bytes(int64_t nv);
int emp_label_mesh_index(const uint64_t *vkeys, int64_t nv, const uint64_t *qkeys, const int32_t *qdirs, int64_t nq,
                         int64_t H, int64_t W, void *work, int64_t work_bytes, int32_t *vertices, int32_t *quads,
                         int64_t *objects, int64_t max_objects, int32_t *n_objects, void *stream);
int emp_mesh_neighbours(const int32_t *vertices, int64_t nv, const int32_t *quads, int64_t nq, int32_t *nbr,
                        void *stream);
int emp_mesh_smooth(const float *src, const int32_t *nbr, int64_t nv, float factor, float *dst, void *stream);

/* ---- E8: skeletons of a label volume (thinning that keeps 1-D isthmuses, by sub-fields) and their graph -------------
 * replaces, on the device, what users of the reference run on a CPU after the fact, object by object: kimimaro or
 *          skimage.morphology.skeletonize over a volume that was already resident.
 * Setting.  L is a label volume (D, H, W), item = 1 or 4, 0 = background, the bits taken as they are (E2-E7).  The
 *   object of a voxel v is the set of alive voxels with v's label; other labels, deleted voxels, 0 and positions outside
 *   the volume are background for v.  Every voxel carries two bits: alive, initially L != 0, and kept, initially 0.
 * Neighbourhood mask.  M(v) has 26 bits; bit n is set iff the neighbour at offset (dz, dy, dx) is alive and has v's
 *   label; offsets are numbered in ascending (dz, dy, dx) order from (-1, -1, -1), skipping the centre:
 *   n = 9 (dz + 1) + 3 (dy + 1) + (dx + 1), minus 1 past the centre.
 * Predicates.  c26 = the number of 26-connected components of the set bits (two positions are adjacent iff they differ
 *   by at most 1 in every coordinate).  t6: take the clear bits among the 18 face and edge positions, form components
 *   under 6-adjacency among those 18 positions, count those that contain one of the 6 face positions.  v is SIMPLE iff
 *   c26 = 1 and t6 = 1 (Bertrand-Malandain, (26, 6)); v is an ISTHMUS iff c26 >= 2.
 * Schedule.  Iteration k = 1, 2, ...:
 *   1. Mark.  Every alive voxel with a face neighbour that is not in its object is marked as border for this iteration.
 *   2. Sub-fields.  For s = 0 .. 7 in this order, s = (Z & 1) << 2 | (y & 1) << 1 | (x & 1), Z the GLOBAL slice number
 *      z_base + z: every voxel of sub-field s that is alive, marked and not kept is examined on the current state.  An
 *      isthmus is set kept (for good; it stays), else a simple voxel is deleted, else it stays as it is and may be
 *      examined again in a later iteration.
 *   3. Stop after the first iteration in which no voxel was deleted, on any block or rank.
 *   Two voxels of one sub-field are never 26-adjacent, so the decisions of a pass do not depend on one another or on
 *   their order: the parallel schedule equals the sequential one, and in-place byte stores are race-free.
 * Result.  S = alive ? L : 0.  S is a subset of L; per label the 26-components, enclosed cavities and tunnels are those
 *   of L; a ball ends as one voxel; a solid with a cavity keeps a closed shell around it.  NOT idempotent: thinning S
 *   again starts with no kept voxel and eats the curves from their ends.
 * emp_skel_classify   out[i] = bit 0 simple | bit 1 isthmus of masks[i] (bits 26 .. 31 ignored): the device function
 *                     that the pass uses.
 * `state` is one uint8 per voxel, owned by the caller: bit 0 alive, bit 1 kept, bit 2 this iteration's mark.  It is
 * the interface between passes, z-blocks and ranks.  `work` (emp_label_thin_work_bytes; -1 for a shape that a call
 * would refuse) holds the list of tiles (8 x 8 x 64 voxels) that hold a labelled voxel, two byte arrays of due tiles
 * and the counters: uint64 at work + 0 = length of the list, at work + 8 = voxels deleted since the initialisation,
 * the only atomic of the passes.  Layout, every part on the next multiple of 256 bytes, n = ceil(D / 8) ceil(H / 8)
 * ceil(W / 64) tiles: the two counters; list, n int32; n bytes, 1 = the tile is due for the next mark; n bytes, 1 = the
 * tile is due for the passes (written by the mark step, cleared by a pass that leaves no candidate).  A call covers at most 2^31 - 1 voxels; every argument error is EMP_EINVAL before any
 * launch; D == 0 is a no-op.  below / above: ONE slice each of (labels, state) of the neighbouring z-block or rank,
 * both null = the volume's face.
 * emp_label_thin_init   writes every state byte, the list, and marks every listed tile as due for the first mark.
 * emp_label_thin_mark   step 1 over the due tiles, one workgroup per listed tile (n_listed = the list's length): a tile
 *                       is due when a voxel of it or of its ring was deleted since it was last marked; force bit 0 / 1
 *                       runs the tiles on the first / last slice whatever the flags say (the halo may have changed).
 *                       A tile that then holds no alive, marked, not-kept voxel is not due for the passes.
 * emp_label_thin_pass   step 2 for one sub-field, one workgroup per listed tile; tile and ring are staged in LDS.  A
 *                       deletion makes the tile and every tile whose ring holds the voxel (faces, edges, corners) due
 *                       for the next mark.
 * emp_label_thin_paint  dst = alive ? L : 0 over n voxels, item size 1 or 4; dst may be the labels themselves.
 * Graph of a sparse label volume S (whatever made it).  Vertices: every voxel with S != 0, key = label << 32 | global
 *   voxel number ((z_base + z) H + y) W + x, ascending by (label unsigned, z, y, x).  Edges: one per unordered pair of
 *   26-adjacent voxels of one label, owned by the lower voxel, for the 13 offsets lexicographically above (0, 0, 0),
 *   codes 0 .. 12 in ascending (dz, dy, dx); ascending by (label, lower voxel, code).  A block owns the edges whose lower
 *   end it owns, so edges need only `above`; the degree of a vertex, the number of its 26-neighbours of its label, is
 *   read at emit time and needs both.
 * Step 1  emp_label_graph_count: R = D H rows; row_offsets[0 .. 2 R] (2 R + 1 int32) = exclusive prefix sum of the
 *         vertices per row, then of the edges per row: row_offsets[R] = nv, row_offsets[2 R] - nv = ne.  D H W <= 2^26
 *         per call.  work: emp_label_graph_count_work_bytes(R) bytes.
 * Step 2  emp_label_graph_emit: vkeys / vdeg (nv) in voxel order, ekeys = label << 32 | lower voxel / ecodes (ne) in
 *         (voxel, code) order; an item past the totals is dropped, never written.
 * Step 3  the caller sorts both key arrays stably over bits 32 .. 63 (emp_sort_u64_i32), blocks and ranks concatenated
 *         in z order first; vertex attributes travel as a sorted permutation.
 * Step 4  emp_label_graph_index: vertices (nv, 3) int32 zyx global, edges (ne, 2) int32 with i < j, each end found by
 *         binary search inside its object's [v_begin, v_end), -1 where the keys hold no such vertex; objects (n, 8)
 *         int64: label, v_begin, v_end, e_begin, e_end, isolated (degree 0), ends (degree 1), junctions (degree >= 3);
 *         at most max_objects rows are written, n_objects (device int32) receives the number of labels.  work:
 *         emp_label_graph_index_work_bytes(nv) bytes.
 * No step of the graph uses atomics: bit-identical from run to run and from any z-partition.  Refused, never truncated:
 * a whole volume above 2^32 voxels, nv or ne of 2^31 or more.                                                        */
int emp_skel_classify(const uint32_t *masks, int64_t n, uint8_t *out, void *stream);
int64_t emp_label_thin_work_bytes(int64_t D, int64_t H, int64_t W);
int emp_label_thin_init(const void *lab, int item, int64_t D, int64_t H, int64_t W, uint8_t *state, void *work,
                        int64_t work_bytes, void *stream);
int emp_label_thin_mark(const void *lab, int item, int64_t D, int64_t H, int64_t W, uint8_t *state,
                        const void *below_lab, const uint8_t *below_state, const void *above_lab,
                        const uint8_t *above_state, void *work, int64_t work_bytes, int64_t n_listed, int force,
                        void *stream);
int emp_label_thin_pass(const void *lab, int item, int64_t D, int64_t H, int64_t W, uint8_t *state,
                        const void *below_lab, const uint8_t *below_state, const void *above_lab,
                        const uint8_t *above_state, void *work, int64_t work_bytes, int64_t n_listed, int subfield,
                        int64_t z_base, void *stream);
int emp_label_thin_paint(const uint8_t *state, const void *lab, int item, int64_t n, void *dst, int dst_item,
                         void *stream);
int64_t emp_label_graph_count_work_bytes(int64_t R);
int emp_label_graph_count(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below,
                          const void *above, void *work, int64_t work_bytes, int32_t *row_offsets, void *stream);
int emp_label_graph_emit(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, const void *above,
                         int64_t z_base, const int32_t *row_offsets, int64_t nv, int64_t ne, uint64_t *vkeys,
                         int32_t *vdeg, uint64_t *ekeys, int32_t *ecodes, void *stream);
int64_t emp_label_graph_index_work_bytes(int64_t nv);
int emp_label_graph_index(const uint64_t *vkeys, const int32_t *vdeg, int64_t nv, const uint64_t *ekeys,
                          const int32_t *ecodes, int64_t ne, int64_t H, int64_t W, void *work, int64_t work_bytes,
                          int32_t *vertices, int32_t *edges, int64_t *objects, int64_t max_objects, int32_t *n_objects,
                          void *stream);

/* ---- E9: contact sites between labelled objects -- a table of the pairs that lie within a radius of each other ----------
 * replaces, on the device, what users of the reference run on a CPU after the fact, object pair by object pair:
 *          scipy.ndimage.distance_transform_edt or a dilation per object, then a comparison with every other object.
 * Setting.  A and B are label volumes (D, H, W) of equal shape, each with item = 1 (uint8) or 4 (uint32; the bits of an
 *   int32 are taken as they are, as in E2-E8); 0 is background.  B may be A itself (same = 1).  The voxel pitch
 *   (az, ay, ax) is integers in 1 .. 16; r2 is an integer with min(pitch)^2 <= r2 and isqrt(r2) / min(pitch) <= 4
 *   (CONTACT_MAX_HALO).  Anything else is refused.
 * Ball.  The offsets o = (dz, dy, dx) with d2(o) = az^2 dz^2 + ay^2 dy^2 + ax^2 dx^2 <= r2, in ascending (d2, dz, dy,
 *   dx); (0, 0, 0) is one of them; at unit pitch and r2 = 24 there are 485.  Nothing lies outside the volume: its faces
 *   hold no candidates (as in E5).
 * Contact voxel.  v is a contact voxel of the ordered pair (a, b) when A(v) = a != 0, b != 0, b != a in the same-volume
 *   case, and some offset o of the ball has B(v + o) = b.  Its distance d2(v, b) is the smallest such d2(o).  One voxel
 *   may be a contact voxel of many b; all of them count, not only the nearest.  With two volumes a voxel may be labelled
 *   in both: d2 = 0, a contact.
 * Table.  One row of 10 int64 per ordered pair (a, b) with at least one contact voxel, ascending by (a, b) as unsigned
 *   32-bit values: a, b, voxels, min_d2, sum_z, sum_y, sum_x, faces_z, faces_y, faces_x.  voxels: the contact voxels of a
 *   with b; min_d2: the smallest d2(v, b) among them; sum_*: their index sums, z_base added to z; faces_i: over those
 *   voxels, the number of 6-neighbours along axis i that carry b in B, counted only when a_i^2 <= r2 (that neighbour
 *   lies in the ball; with r2 >= max(pitch)^2 that is every a|b face).  Columns 2 and 4..9 are sums, column 3 is a
 *   minimum, and every contact voxel belongs to the one z-block that owns v: tables of z-blocks and ranks merge exactly,
 *   whatever the partition and the order.  In the same-volume case min_d2 and faces_* of (a, b) equal those of (b, a).
 *   All results are exact integers, bit-identical from run to run and from any z-partition.
 * The volume B may be continued along z by two halo stacks as in E5: `below` holds hb slices that stand for z = -hb ..
 *   -1 and `above` ha slices for z = D .. D + ha - 1, of B's item size, hb, ha <= isqrt(r2) / az; 0 = the volume's face.
 * ball: the table above on the device, n_ball rows of 4 int32 (dz, dy, dx, d2), built by the caller; a row that reaches
 *   outside the ring (isqrt(r2) / pitch per axis) or whose d2 is not in 0 .. r2 is not walked, so no table makes a kernel
 *   read outside its tile.
 * Step 1  emp_label_contacts_count: flags the tiles (8 x 8 x 64 voxels) in which A has a label and B's tile plus ring
 *         holds a possible partner, lists them, counts the records of every listed tile -- one per (contact voxel, b) --
 *         and scans the counts.  totals (device int64[2]) receives the listed tiles and the records.  All of it stays in
 *         `work` (emp_label_contacts_work_bytes; -1 for a shape that a call would refuse) for step 2.  A call covers at
 *         most 2^31 - 1 voxels.
 * Step 2  emp_label_contacts_emit: the same walk writes per record keys = a << 32 | b, vox = the voxel's number inside
 *         the block and d2f = d2 << 6 | six face bits (bit 2 axis + side).  n_records >= 2^31 is refused, never
 *         truncated: the caller cuts a smaller z-block.  The order of a tile's records is not fixed; the table is.
 * Step 3  the caller sorts the keys over all 64 bits with emp_sort_u64_i32, carrying the permutation 0 .. n - 1.
 * Step 4  emp_label_contacts_rows: heads of the runs of equal sorted keys and their scan, kept in `work`
 *         (emp_label_contacts_rows_work_bytes); n_rows (device int32) receives the number of rows.
 * Step 5  emp_label_contacts_reduce: with the same `work`, writes the n_rows rows of `table`; the sums and the minimum
 *         are integer atomics, so no order shows in them.                                                             */
int64_t emp_label_contacts_work_bytes(int64_t D, int64_t H, int64_t W);
int emp_label_contacts_count(const void *a, int item_a, const void *b, int item_b, int64_t D, int64_t H, int64_t W,
                             const void *below, int64_t hb, const void *above, int64_t ha, int same, int az, int ay,
                             int ax, int r2, const int32_t *ball, int n_ball, void *work, int64_t work_bytes,
                             int64_t *totals, void *stream);
int emp_label_contacts_emit(const void *a, int item_a, const void *b, int item_b, int64_t D, int64_t H, int64_t W,
                            const void *below, int64_t hb, const void *above, int64_t ha, int same, int az, int ay,
                            int ax, int r2, const int32_t *ball, int n_ball, void *work, int64_t work_bytes,
                            int64_t n_listed, int64_t n_records, uint64_t *keys, int32_t *vox, int32_t *d2f,
                            void *stream);
int64_t emp_label_contacts_rows_work_bytes(int64_t n);
int emp_label_contacts_rows(const uint64_t *keys, int64_t n, void *work, int64_t work_bytes, int32_t *n_rows,
                            void *stream);
int emp_label_contacts_reduce(const uint64_t *keys, const int32_t *perm, const int32_t *vox, const int32_t *d2f,
                              int64_t n, int64_t H, int64_t W, int64_t z_base, const void *work, int64_t work_bytes,
                              int64_t *table, int64_t n_rows, void *stream);

/* ---- E10: local thickness of the labelled objects -- the largest inscribed ball that covers a voxel ---------------------
 * replaces, on the device, what users of the reference run on a CPU after the fact: ImageJ / BoneJ "Local Thickness" or
 *          a loop over the objects with an edt each (Hildebrand and Ruegsegger's definition).
 * Setting.  L is a label volume (D, H, W), item = 1 (uint8) or 4 (uint32; the bits of an int32 are taken as they are),
 *   0 = background.  The voxel pitch (az, ay, ax) is integers in 1 .. 16 and |o|^2 = az^2 dz^2 + ay^2 dy^2 + ax^2 dx^2.
 *   1 <= cap <= 65535.  d2(q) is what emp_label_edt (E5) defines for that cap: 0 on background, otherwise the smallest
 *   |q - u|^2 over the voxels u of the volume with L(u) != L(q), background included, and cap where nothing lies nearer;
 *   positions outside the volume are no candidates.
 * Definition.  T2(p) = max { d2(q) : q in the volume, |p - q|^2 < d2(q) }, 0 if there is no such q: the squared radius
 *   of the largest ball, centred anywhere, that fits its object and covers p.  All quantities are exact integers and
 *   the result does not depend on how it is computed.
 *   - T2(p) > 0 exactly where L(p) != 0, and T2 >= d2 (q = p covers p).
 *   - No label test is needed: every p with |p - q|^2 < d2(q) carries q's label by the definition of d2, so a ball
 *     never leaks into a touching object, and the volume's faces do not thin an object.
 *   - The cap is part of the definition: the result for cap is NOT min(T2 without a cap, cap).  A ball whose true
 *     radius exceeds the cap is shrunk to the cap and covers less.  totals[1] counts the voxels with d2 == cap; when it
 *     is 0 the result is the uncapped one.
 *   - The diameter at p is 2 sqrt(T2(p)) in pitch units, with the voxel-centre bias of the edt: a line one voxel wide
 *     reads 2.  Nothing corrects for it.
 * The volume may be continued along z by two halo stacks as in E5: `below` holds hb >= 0 slices that stand for z = -hb
 *   .. -1 and `above` ha >= 0 slices for z = D .. D + ha - 1; 0 = the volume's face.  d2 is computed over the EXTENDED
 *   volume of hb + D + ha slices, whose end slices are faces, and T2 is written for the D slices of lab.  With h =
 *   floor(sqrt(cap - 1)) / az, T2 of the core needs d2 on h slices per side and that d2 needs labels on h more: 2 h
 *   slices per side make every z-partition equal the undivided volume, with no table, seam or merge.  With fewer, the
 *   result is that of the truncated volume.
 * The three steps share `work` (emp_label_thick_work_bytes; -1 for a shape a call would refuse): 8 bytes per voxel of
 *   the extended volume and a few words per tile of 8 x 8 x 64 voxels.  Kernels initialise all of it.  A call covers at most
 *   2^31 - 1 voxels, halos included; a larger block and every other argument error is refused with EMP_EINVAL before
 *   any launch, nothing is truncated.  D == 0 is a no-op (totals are zeroed).
 * Step 1  emp_label_thick_edt: d2 of every voxel of the extended volume, by the passes of emp_label_edt.
 * Step 2  emp_label_thick_lists: per tile of the extended volume the voxels with d2 > 0 as keys d2 << 12 | voxel in
 *         tile, sorted descending, at the tile's scanned offset, and the tile's largest d2.  totals (device int64[4]):
 *         candidates listed, voxels of the core with d2 == cap, tiles with a list, longest list.
 * Step 3  emp_label_thick_resolve: T2 of the core as (D, H, W) uint16.  A tile's values start as its own d2 and take
 *         the balls of its own list and of every tile whose largest ball can reach it; a maximum, without global
 *         atomics, bit-identical from run to run.                                                                    */
int64_t emp_label_thick_work_bytes(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha);
int emp_label_thick_edt(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, int64_t hb,
                        const void *above, int64_t ha, int az, int ay, int ax, int cap, void *work, int64_t work_bytes,
                        void *stream);
int emp_label_thick_lists(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha, int cap, void *work,
                          int64_t work_bytes, int64_t *totals, void *stream);
int emp_label_thick_resolve(int64_t D, int64_t H, int64_t W, int64_t hb, int64_t ha, int az, int ay, int ax, int cap,
                            const void *work, int64_t work_bytes, uint16_t *out, void *stream);

/* ---- E11: shape descriptors of the labelled objects -- Crofton intercepts, Euler number, second moments -----------------
 * replaces, on the device, what users of the reference run on a CPU after the fact, object by object: MorphoLibJ's
 *          "Analyze Regions 3D" or regionprops (surface area, Euler number, inertia ellipsoid).
 * Setting.  L is a label volume (D, H, W), item = 1 (uint8) or 4 (uint32; the bits of an int32 are taken as they are),
 *   0 = background; everything outside the volume is 0, as in E2, except the two optional neighbour slices `below`
 *   (z = -1) and `above` (z = D), contiguous (H, W) arrays of the same item size (null = 0).  A voxel is p = (z, y, x)
 *   with z counted as z_base + local z.  M(p) is E8's mask of the 26 neighbours of p that carry p's label: bit n stands
 *   for position 9 (dz + 1) + 3 (dy + 1) + (dx + 1) of the 3 x 3 x 3 block, minus 1 past the centre.
 * Definition.  The table has one row of 26 int64 per distinct non-zero label, ascending by label as an unsigned
 *   number; every column after the label is a sum over the voxels p of that label:
 *     0        label
 *     1        voxels                   1
 *     2..4     sum_z, sum_y, sum_x      z, y, x
 *     5..10    sum_zz, sum_yy, sum_xx, sum_zy, sum_zx, sum_yx     the products of the indices
 *     11..23   cross_0 .. cross_12      [L(p + d_k) != L(p)] + [L(p - d_k) != L(p)] for E8's edge code k: d_k is the
 *                                       offset of bit 13 + k of M, i.e. (0,0,1), (0,1,-1), (0,1,0), (0,1,1), (1,-1,-1),
 *                                       (1,-1,0), (1,-1,1), (1,0,-1), (1,0,0), (1,0,1), (1,1,-1), (1,1,0), (1,1,1)
 *     24       corners                  the corners (8) of p's unit cube of which p is the first voxel of its label, in
 *                                       (z, y, x) order, among the 8 voxels around that corner
 *     25       edges                    the same for the 12 edges of p's cube, with 4 voxels around each
 *   cross_k counts the ends of the object's intercepts with the lattice lines of direction d_k (two per intercept),
 *   which is what a Crofton estimate of the surface area needs; background counts as different.  By construction
 *     - columns 1..4 are E2's voxels, sum_z, sum_y, sum_x, and cross_8, cross_2, cross_0 E2's faces_z, faces_y, faces_x;
 *     - the object touches faces = 3 voxels + (cross_8 + cross_2 + cross_0) / 2 lattice faces, `corners` lattice points
 *       and `edges` lattice edges, each counted once: the cells of the cubical complex of its closed voxels;
 *     - euler = corners - edges + faces - voxels is the Euler number of that complex, i.e. of the object as a
 *       26-connected set with 6-connected background: the convention of E8 and of E3 with connectivity 26.
 *   All are sums of integers, so the table of a volume equals the merge (sum per label) of the tables of any
 *   z-partition whose blocks were given their true neighbour slices, and no visiting order shows in the result.
 * Limits, refused with EMP_EINVAL before any launch and never truncated: D * H * W <= 2^31 - 1 per call (cut the slab
 *   into z-blocks), 0 <= z_base, z_base + D <= 2^20, H <= 2^20, W <= 2^20.  The second-order sums are exact while they
 *   stay below 2^63 -- always at 1024^3, in general while (largest index)^2 * voxels of the label < 2^63.  An overflow
 *   beyond that wraps and is NOT detected.
 * Step 1  emp_label_measure_count (E2): the run total n_runs sizes step 2.
 * Step 2  emp_label_shape_labels: the distinct non-zero labels of the block, ascending, as uint32 in `labels`
 *         (capacity n_runs); n_out (device int32[1]) receives their number.  work: emp_label_shape_work_bytes(
 *         n_runs) bytes.
 * Step 3  emp_label_shape: out_table (n_labels, 26) int64, row i for labels[i]; every cell is written.  One pass over
 *         the block by tiles of 8 x 8 x 64 voxels; a tile without a label costs the read of its own voxels.  counters
 *         (device int64[2]): tiles that hold a label, voxels whose sums went to the table directly because their tile
 *         held more labels than the tile's table has slots.  A label of the block that is missing in `labels` is
 *         skipped, never written elsewhere.  Integer atomics only: bit-identical from run to run.  n_labels == 0 or
 *         D == 0 zeroes the counters and returns.                                                                    */
int64_t emp_label_shape_work_bytes(int64_t n_runs);
int emp_label_shape_labels(const void *lab, int item, int64_t D, int64_t H, int64_t W, const int32_t *row_offsets,
                           int64_t n_runs, void *work, int64_t work_bytes, uint32_t *labels, int32_t *n_out,
                           void *stream);
int emp_label_shape(const void *lab, int item, int64_t D, int64_t H, int64_t W, const void *below, const void *above,
                    int64_t z_base, const uint32_t *labels, int64_t n_labels, int64_t *out_table, int64_t *counters,
                    void *stream);

/* ---- T1 on the device: run table of a plane's slices -> per-instance 3D runs sorted by (instance, start) ------
 * replaces InstanceTracker.update / finish        empanada/inference/tracker.py:61-123
 *          to_coords3d                             empanada/inference/tracker.py:25-38
 * and feeds merge_objects_from_trackers (empanada/consensus.py:348-469) and the fill without a host round trip.
 * A 3D run is (key, len): key = instance << 40 | flat (z, y, x) start of the (Z, Y, X) volume; len in voxels.
 * comp_inst[c] = instance index of component c of the run table (its position in the tracker's dict order), -1 =
 * skip (halo slice, removed).  inst_base is added to every instance index (planes concatenated for the consensus).
 *
 * emp_track_lift  axis 0 (xy: plane (H, W) = (Y, X), slices along z): start3d = start + slice * Y * X;
 *                 axis 1 (xz: plane (H, W) = (Z, X), slices along y): start3d = (start / W) * Y * X + slice * X +
 *                 start % W -- only the START is mapped and the length kept, reproducing the row wrap of
 *                 tracker.py:78-82.  Runs of one instance that are contiguous inside a slice are merged first (what
 *                 rle_encode over the instance's pixels yields, array_utils.py:209-235).  slice = c_slice + slice0.
 *                 Outputs hold at most n_runs entries; n_out is a device int32.  work: emp_track_work_elems(n_runs)
 *                 int32.
 * emp_track_lift_yz  for the yz plane the tracker is the run-length encoding along x of the dense labelling
 *                 (tracker.py:83-88,110-113): scatter instance + 1 with emp_scatter_yz_u32 into a (Z, Y, Xl) volume,
 *                 extract its row runs (emp_runs_count / _extract) and pass them here: start3d = row * X + x0 + x.
 * emp_track_sort  stable radix sort by key; with merge_touching, runs of one instance whose previous end equals their
 *                 start are joined (np.sort + rle_encode in tracker.finish).  Any of out_key / out_st (= key's low 40
 *                 bits) may be NULL.  work: emp_track_sort_work_bytes(n) bytes.
 * emp_track_offsets  CSR offsets of the instances in a sorted key array: out_off[k] = first run with instance >= k,
 *                 k = 0 .. n_inst.
 * emp_track_expand  out[i] = obj_val[instance that owns run i] (vote groups, fill order) from CSR offsets.
 * emp_track_clip  the part of every run inside the flat interval [lo, hi): a rank's z-slab of the output volume
 *                 (chunk_ranges, empanada/zarr_utils.py:11-47, splits runs at chunk borders the same way).
 *                 work: emp_track_work_elems(n) int32.                                                        */
int64_t emp_track_work_elems(int64_t n_runs);
int emp_track_lift(int axis, const int32_t *r_start, const int32_t *r_len, const int32_t *r_comp,
                   const int32_t *c_slice, const int32_t *comp_inst, int64_t n_runs, int H, int W, int Y, int X,
                   int slice0, int64_t inst_base, int32_t *work, uint64_t *out_key, int64_t *out_len,
                   int32_t *n_out, void *stream);
/* emp_tile_lift  C5, Tiler.translate_rle_seg (empanada/inference/tile.py:122-168) for all slices of one tile: runs of
 *                 every object merged as rle_encode of its flat TILE indices merges them, start mapped into the image
 *                 frame ((start / tw + y0) * X + start % tw + x0), length kept; 2D positions, the slice stays with the
 *                 object: key = (inst_base + comp_inst[comp]) << 40 | start2d.  work: emp_track_work_elems(n_runs). */
int emp_tile_lift(const int32_t *r_start, const int32_t *r_len, const int32_t *r_comp, const int32_t *c_slice,
                  const int32_t *comp_inst, int64_t n_runs, int tw, int X, int y0, int x0, int64_t inst_base,
                  int32_t *work, uint64_t *out_key, int64_t *out_len, int32_t *n_out, void *stream);
int emp_track_lift_yz(const int32_t *row_offsets, const int32_t *r_start, const int32_t *r_len,
                      const uint32_t *r_val, int64_t n_rows, int64_t n_runs, int Xl, int X, int x0,
                      int64_t inst_base, uint64_t *out_key, int64_t *out_len, void *stream);
int64_t emp_track_sort_work_bytes(int64_t n);
int emp_track_sort(const uint64_t *key_in, const int64_t *len_in, int64_t n, int merge_touching, void *work,
                   int64_t work_bytes, uint64_t *out_key, int64_t *out_st, int64_t *out_len, int32_t *n_out,
                   void *stream);
int emp_track_offsets(const uint64_t *keys_sorted, int64_t n, int64_t n_inst, int64_t *out_off, void *stream);
int emp_track_expand(const int64_t *off, const int32_t *obj_val, int64_t n_obj, int64_t n_runs, int32_t *out,
                     void *stream);
int emp_track_clip(const uint64_t *key, const int64_t *len, int64_t n, int64_t lo, int64_t hi, int32_t *work,
                   uint64_t *out_key, int64_t *out_len, int32_t *n_out, void *stream);

/* ---- M4/M5 (host): slice-to-slice label propagation over component tables, plain C++ on the CPU ---------
 * replaces RLEMatcher.__call__ driven by forward_matching / backward_matching
 *          empanada/inference/matcher.py:262-323, inference/patterns.py:60-121
 * for the whole-stack path, where the GPU has already reduced every slice to connected components
 * (emp_runs_label) and their overlaps with the next slice (emp_runs_overlap_next).  One call per class.
 * Components sorted by (slice, cc label): slice t owns [bounds[t], bounds[t+1]); pa / pb are positions inside
 * slice t / t+1 of the overlap triplets [tb_bounds[t], tb_bounds[t+1]).  IoU fp64, IoA fp32, thresholds and merge
 * rule as in the reference; the Hungarian step runs only when an overlap matrix has a row or column with two
 * non-zeros and is delegated to `lsap` (the caller passes scipy.optimize.linear_sum_assignment(maximize=True),
 * the routine the reference calls, so ties break identically): lsap(iou row-major, n_rows, n_cols, rows_out,
 * cols_out) -> number of pairs or -1.
 * comp_final[n]: final label per component (sorted order); seen_labels / n_seen: labels in order of first update
 * when slices are visited last to first (the tracker's dict order).
 * Returns 0; 1 where the reference raises ValueError (ioa_thr <= 0 and an empty target slice); 2 lsap failed.  */
typedef int64_t (*emp_lsap_fn)(const double *iou, int64_t n_rows, int64_t n_cols, int64_t *rows_out,
                               int64_t *cols_out);
/* lsap == NULL: the library's own restatement of that routine (emp_lsap_maximize: shortest augmenting paths after
 * Crouse 2016 with scipy 1.15's column order and tie rule, checked against scipy itself by
 * tests/test_sharded_gloo.py::test_native_lsap_equals_scipy) -- no Python in the loop. */
int64_t emp_lsap_maximize(const double *cost, int64_t n_rows, int64_t n_cols, int64_t *rows_out, int64_t *cols_out);
int emp_chain_class(int64_t D, const int64_t *bounds, const int64_t *comp_label, const int64_t *comp_area,
                    int is_thing, const int64_t *tb_bounds, const int64_t *pa, const int64_t *pb,
                    const int64_t *tv, int64_t class_id, int64_t label_divisor, double iou_thr, double ioa_thr,
                    emp_lsap_fn lsap, int64_t *comp_final, int64_t *seen_labels, int64_t *n_seen);

/* ---- D10: PointRend subdivision step (eval branch) ---------------------------------------------------------------
 * replaces, per render step of the exported models' `forward(x, render_steps, interpolate_ins)`:
 *   F.interpolate(x2, bilinear, align_corners=False)       empanada/models/point_rend.py:244-245
 *   calculate_uncertainty + get_uncertain_point_coords_on_grid (torch.topk)   point_rend.py:62-79,97-125
 *   point_sample (F.grid_sample, bilinear, align_corners=False, zeros) of features and coarse logits   :35-60,253-254
 *   StandardPointHead (Conv1d + ReLU x num_fc, predictor; coarse logits re-fed to every layer)          :138-190
 *   scatter_ of the point predictions into the upsampled logits                                          :258-265
 * emp_pr_upsample2x  logits (N, C, h, w) planar -> out (N, C, 2h, 2w) and uncertainty (N, 4hw): -|l| for C == 1,
 *                    second-largest minus largest logit otherwise.
 * emp_pr_topk        idx (N, k) int32 = pixel indices of the k largest uncertainties of every image: exact (radix
 *                    select); ties at the k-th value go to the lowest indices; order: the strictly larger ones in pixel
 *                    order, then the ties in pixel order.  work: emp_pr_topk_work_bytes(N, HW) bytes.
 * emp_pr_point_sample  features NHWC (N, Hf, Wf, CF), pixel stride feat_pixel_stride; coarse (N, C, Hf, Wf) planar;
 *                    point p = n * k + j sits at the centre of pixel idx[p] of the (H, W) grid.  Writes row p of the
 *                    MLP input matrix X0 (P, ld): channels [0, CF) sampled features, [CF, CF + C) sampled coarse logits,
 *                    [CF + C, ld) zeros; and the channels [CF, ld) of X1 (the next layer's input, whose first CF
 *                    channels the MLP layer writes).  ld % 16 == 0 so that emp_conv_bn_act_nhwc can consume it.
 * the MLP            emp_conv_bn_act_nhwc(x = X as (1, P, 1, ld), w = (Cout, 1, 1, ld) zero-padded, shift = bias,
 *                    relu, out = channel slice [0, Cout) of the other matrix): summation order of D4.
 * emp_pr_scatter     logits[n, c, idx[p]] = points[p * ld_points + c].                                            */
int emp_pr_upsample2x(const float *logits, int N, int C, int h, int w, float *out, float *uncertainty, void *stream);
int64_t emp_pr_topk_work_bytes(int N, int64_t HW);
int emp_pr_topk(const float *uncertainty, int N, int64_t HW, int k, void *work, int64_t work_bytes, int32_t *idx,
                void *stream);
int emp_pr_point_sample(const float *feat_nhwc, int64_t feat_pixel_stride, const float *coarse, int N, int Hf, int Wf,
                        int CF, int C, const int32_t *idx, int k, int H, int W, float *X0, float *X1, int ld,
                        void *stream);
int emp_pr_scatter(const float *points, int ld_points, const int32_t *idx, int N, int C, int k, int64_t HW,
                   float *logits, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EMP_HIP_H */
