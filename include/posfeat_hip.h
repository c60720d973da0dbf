/*
 * posfeat_hip.h -- C ABI of libposfeat_hip.so, the MI355X (gfx950) engine for
 * the PoSFeat extraction + correlation hot path.
 *
 * The reference (The-Learning-And-Vision-Atelier-LAVA/PoSFeat) has no FFI: its
 * hot path is duck-typed Python over PyTorch ATen.  Each entry point below
 * replaces the ATen work behind one reference Python surface (cited), and the
 * Python shims in posfeat_amd/ (networks/, losses/, managers/) keep those
 * surfaces' names, argument meanings and error behaviour.
 *
 * Conventions
 *   - All pointers are device pointers unless stated; all tensors are
 *     caller-owned (the library never allocates device memory except inside
 *     posfeat_model_create, which allocates nothing either: the caller passes
 *     workspace).  Scratch comes from a caller workspace sized by *_workspace.
 *   - `stream` is a hipStream_t passed as void*; every call is stream-ordered
 *     and never synchronises the host (graph-capturable), except where noted.
 *   - Return 0 on success or a negative POSFEAT_E_* code; posfeat_strerror()
 *     describes it.  No C++ exception crosses the ABI.
 *   - Feature maps inside the engine are NHWC fp32 with an explicit pixel
 *     stride (`*_cstride`, in floats) so channel concatenation is free.
 */
#ifndef POSFEAT_HIP_H
#define POSFEAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POSFEAT_OK 0
#define POSFEAT_E_INVALID (-1)     /* bad argument / unsupported shape     */
#define POSFEAT_E_HIP (-2)         /* a HIP runtime call failed            */
#define POSFEAT_E_WORKSPACE (-3)   /* workspace too small                  */
#define POSFEAT_E_UNSUPPORTED (-4) /* option the engine does not implement */

#define POSFEAT_ACT_NONE 0
#define POSFEAT_ACT_RELU 1
#define POSFEAT_ACT_ELU 2

const char *posfeat_strerror(int code);
int posfeat_abi_version(void);
/* 1 if a gfx950 device is visible and the code object loads on it. */
int posfeat_device_ok(void);

/* ------------------------------------------------------------------------
 * Fused convolution (implicit GEMM on v_mfma_f32_32x32x2_f32).
 * Replaces: nn.Conv2d + eval BatchNorm2d + ReLU/ELU (+ residual add) of
 *   networks/DescNet.py:167-179 (conv), 182-190 (upconv's conv) and the
 *   torchvision Bottleneck convs behind DescNet.py:27-35; and the bias-only
 *   convs of networks/DeteNet.py:11-21.
 * x: NHWC, pixel stride x_cstride >= cin (cin multiple of 4); cout, y/res
 *    strides multiple of 4 and x/w/y/res/bias 16-B aligned (vector epilogue).
 * w: packed [cout][Kpad], K ordered (kh, kw, cin), Kpad = roundup(K, 32),
 *    zero-padded (posfeat_conv_packed_k).  BN already folded into w/bias.
 * y[p, c] = act(sum + bias[c] + res[p, c])   (res may be NULL)
 * ------------------------------------------------------------------------ */
typedef struct {
  int n, h, w;       /* input batch / height / width                      */
  int cin;           /* input channels, multiple of 4                     */
  int x_cstride;     /* floats between consecutive input pixels           */
  int cout, kh, kw, stride, pad;
  int y_cstride;     /* floats between consecutive output pixels          */
  int res_cstride;   /* floats between consecutive residual pixels        */
  int act;           /* POSFEAT_ACT_*                                     */
} posfeat_conv_desc;

int posfeat_conv_packed_k(int cin, int kh, int kw); /* returns Kpad */
/* Product arithmetic of the row-tile convolutions (1x1, strided, the batched
 * Winograd / tap GEMMs); returns the previous mode.  0: fp32-input MFMA
 * (v_mfma_f32_32x32x2_f32, exact fp32 fmaf chains).  1 (default): "bf16x6" --
 * each fp32 operand split exactly into three bf16 terms (h + m + l, residual
 * <= 2^-27 relative) and the six products of order >= 2^-16 accumulated in
 * fp32 on v_mfma_f32_32x32x16_bf16 (16x the fp32-MFMA rate): per-product error
 * ~2e-8 relative, below an fp32 fmaf's own rounding -- fp32-accurate results
 * (tests/test_gpu_precision.py), not a reduced-precision mode.  2: as 1, with
 * the Winograd / tap GEMM operands split by their producers (A/B only).
 * 3x3 stride-1 convs with Cin % 32 == 0 and weight planes (the extraction
 * engine's) run the bf16x6 gathered-tap tile in modes >= 1; the fp32 halo
 * kernel is kept for convs without planes and inside the training
 * instances' scopes.  Modes >= 1 also switch DiskLoss's flash passes
 * (posfeat_disk_loss, posfeat_disk_flash_lse) to bf16x6 similarity products.
 * Instances created afterwards plan with the new mode.  mode = -1: query
 * only. */
int posfeat_set_conv_precision(int mode);
/* 1 when this library is the A/B build (`make ab`, libposfeat_hip_ab.so),
 * which reads the POSFEAT_* environment switches that select the non-default
 * paths kept for A/B tests; 0 for the shipped library, which ignores them. */
int posfeat_ab_build(void);
int posfeat_conv2d_nhwc(const posfeat_conv_desc *d, const float *x, const float *w,
                        const float *bias, const float *res, float *y, void *stream);
/* Same, allowed to split K over workgroups (deterministic: fp32 partial slabs
 * summed in split order by a second kernel) when the tile count would leave
 * the last wave of workgroups underfilled.  Scratch: *_workspace bytes
 * (0 = this shape never splits). */
size_t posfeat_conv2d_workspace(const posfeat_conv_desc *d);
int posfeat_conv2d_nhwc_ws(const posfeat_conv_desc *d, const float *x, const float *w,
                           const float *bias, const float *res, float *y, void *ws,
                           size_t ws_bytes, void *stream);
/* Same as posfeat_conv2d_nhwc_ws with the weights ALSO given as their three
 * bf16 planes (h, m, l of the packed [cout][Kpad] array, plane stride wplane
 * elements, >= cout * posfeat_conv_packed_k(cin, kh, kw) or POSFEAT_E_INVALID;
 * h = RNE_bf16(w), m = RNE_bf16(w - h), l = RNE_bf16(w - h - m)),
 * as the engine passes them: the pre-split tiles run (dense 1x1 convs: the
 * 16x16x32 conv_bf6x_kernel; others: conv_bf6d_kernel).  tile: -1 for the
 * default plan, else a tile id the engine's autotuner may pick (ignored where
 * illegal) -- every legal tile of a conv gives bit-identical results.
 * Replaces the same reference convs as posfeat_conv2d_nhwc
 * (networks/DescNet.py:167-190). */
int posfeat_conv2d_nhwc_planes(const posfeat_conv_desc *d, const float *x, const float *w,
                               const unsigned short *wb, long long wplane, const float *bias,
                               const float *res, float *y, void *ws, size_t ws_bytes, int tile,
                               void *stream);
/* The launch plan posfeat_conv2d_nhwc_ws (wplanes = 0) or
 * posfeat_conv2d_nhwc_planes (wplanes = 1) would take for d with every
 * workspace it asks for and the given tile argument, for the calling thread
 * at the current conv precision.  Host only: needs no device, launches
 * nothing.  POSFEAT_E_INVALID for a descriptor the convs reject. */
typedef struct {
  int tile;           /* tile id launched (after any substitution)         */
  int variant;        /* kernel instantiation (conv_plan.h ConvVariant)    */
  const char *kernel; /* its name, a static string                         */
  int bm, bn;         /* output rows / columns per workgroup               */
  int ksplit;         /* split-K factor (1: none)                          */
  int grid, block;    /* workgroups (ksplit included), threads per group   */
  int arith;          /* 0: fp32 MFMA products, 1: bf16x6                  */
} posfeat_conv_plan_info;
int posfeat_conv_plan_query(const posfeat_conv_desc *d, int wplanes, int tile,
                            posfeat_conv_plan_info *out);
/* A torchvision Bottleneck's conv3 + downsample branch as ONE GEMM (the
 * reference's ResUNet encoder, networks/DescNet.py:29-35, through torchvision's
 * Bottleneck: relu(bn3(conv3(t)) + bn_ds(conv_ds(x))) with both BatchNorms
 * folded; replaces conv3 and the downsample conv of layer1.0 / layer2.0 /
 * layer3.0): y[n][oh][ow] = act(x1[n][oh][ow] . W1^T + x2[n][oh*s2][ow*s2] .
 * W2^T + bias), K = k1 + k2, bf16x6 products on the 16x16x32 tiles.  x1: rows
 * of k1 channels (pitch x1cs), x2: an h2 x w2 map of k2 channels (pitch x2cs),
 * wb: the three bf16 planes of the [cout][k1 + k2] weights (plane stride
 * cout * (k1 + k2)), bias: the two biases summed.  k1, k2 % 32 == 0,
 * cout % 128 == 0, 16-B aligned pointers, else POSFEAT_E_INVALID. */
int posfeat_conv1x1_dual(int n, int oh, int ow, const float *x1, int x1cs, int k1,
                         const float *x2, int x2cs, int h2, int w2, int s2, int k2, int cout,
                         const unsigned short *wb, const float *bias, int act, float *y, int ycs,
                         void *stream);
/* Conv (no residual, no activation) whose epilogue also reduces per-tile
 * channel sums for InstanceNorm2d (networks/DeteNet.py:12-22): writes y and
 * mean/rstd [n][cout] of y over each image (biased var, rstd=1/sqrt(var+eps)).
 * Needs out-height*out-width >= 128 (returns POSFEAT_E_UNSUPPORTED otherwise). */
size_t posfeat_conv2d_stats_workspace(const posfeat_conv_desc *d);
int posfeat_conv2d_nhwc_stats(const posfeat_conv_desc *d, const float *x, const float *w,
                              const float *bias, float *y, void *ws, size_t ws_bytes,
                              float *mean, float *rstd, float eps, void *stream);

/* KeypointDet's conv2 over cat[F.interpolate(L, x4, bilinear,
 * align_corners=False), G] + InstanceNorm statistics, without materialising
 * the upsampled map.  Replaces networks/DeteNet.py:109-112 (interpolate, cat,
 * conv2, the statistics of norm2).  L: n x H/4 x W/4 x 192 (pitch lcs), the
 * already normalised PReLU(IN(conv1)); G: n x H x W x 64 (pitch gcs),
 * IN(convimg); w_packed/bias: conv2 (256 -> 128, 3x3) packed as for
 * posfeat_conv2d_nhwc (only read by posfeat_conv2_up4_weights);
 * wph: posfeat_conv2_up4_weights_floats() floats (16 phase-combined weight
 * sets + transposed border taps) built from w_packed (rebuild after changing
 * the weights).
 * Writes y (n x H x W x 128, pitch ycs; bias added, no activation) and
 * mean/rstd [n][128] of y (biased var).  H, W multiples of 4, >= 16. */
size_t posfeat_conv2_up4_weights_floats(void);
size_t posfeat_conv2_up4_workspace(int n, int H, int W);
int posfeat_conv2_up4_weights(const float *w_packed, float *wph, void *stream);
int posfeat_conv2_up4(int n, int H, int W, const float *L, int lcs, const float *G, int gcs,
                      const float *wph, const float *w_packed, const float *bias, float *y,
                      int ycs, void *ws, size_t ws_bytes, float *mean, float *rstd, float eps,
                      void *stream);

/* ------------------------------------------------------------------------
 * Keypoint selection.
 * Replaces: losses/preprocess_utils.py:215-278 generate_kpts_single
 *   (stable=True) with nms (449-464), threshold (232-240), 3x3 soft-argmax
 *   refine + 3x3 max score (242-247), num_pts clamp (249-261), topk+gather
 *   (263-267).
 * kp_map: b x h x w fp32 (the 1-channel local_point).  Tie rule: NMS keeps
 *   p iff S[p] > every earlier and >= every later element of its
 *   reflect-padded window (row-major); top-k orders by (score desc, inner
 *   flat index asc).
 * thr_mode: 0 = no threshold (thr=False), 1 = 'abs', 2 = 'max', 3 = 'mean'.
 * num_pts <= 0 means "all survivors" (num_pts=False).
 * Outputs (capacity `cap` rows per image, cap >= max(num_pts,128) or h*w):
 *   idx [b][cap] int32 inner flat index, coord [b][cap][2] normalised (x,y),
 *   score [b][cap], n_sel[1] (device int32) = rows valid per image (same for
 *   all images, as in the reference), counts[b] (device int32) survivors.
 * ------------------------------------------------------------------------ */
int posfeat_detect_workspace(int b, int h, int w, int cap, size_t *bytes);
int posfeat_detect(const float *kp_map, int b, int h, int w, int nms_radius, int use_nms,
                   int thr_mode, float thr, int num_pts, int cap, int32_t *idx, float *coord,
                   float *score, int32_t *n_sel, int32_t *counts, void *ws, size_t ws_bytes,
                   void *stream);

/* posfeat_detect with every image of the batch selected as if it were
 * detected alone: n_sel[b] (device int32), n_sel[i] = clamp(min(num_pts,
 * counts[i]), 128) -- the reference's extraction loop, which runs
 * generate_kpts_single on one image at a time (extractor.py:336-342 with
 * batch_size 1), for a group of same-size images in one call. */
int posfeat_detect_each(const float *kp_map, int b, int h, int w, int nms_radius, int use_nms,
                        int thr_mode, float thr, int num_pts, int cap, int32_t *idx,
                        float *coord, float *score, int32_t *n_sel, int32_t *counts, void *ws,
                        size_t ws_bytes, void *stream);

/* NMS mask alone (losses/preprocess_utils.py:449-464 nms): mask[b][h][w] = 1
 * iff the pixel is its reflect-padded (2r+1)^2 window's first-occurrence max. */
int posfeat_nms_mask(const float *score, int b, int h, int w, int radius, uint8_t *mask,
                     void *stream);

/* ------------------------------------------------------------------------
 * Descriptor sampling.
 * Replaces: losses/preprocess_utils.py:40-53 sample_feat_by_coord
 *   (grid_sample bilinear, zeros padding, align_corners=False, then
 *   F.normalize p=2 dim=1 eps 1e-12 when `normalize`).
 * fmap: NHWC [b][h][w] with pixel stride cstride, c channels (c <= 1024).
 * coord: [b][npts][2] normalised (x, y); n_valid: optional device int32
 *   (rows beyond *n_valid are written as zeros); out: [b][npts][c].
 * npts == 0 is valid and launches nothing (coord and out, empty, may be null).
 * ------------------------------------------------------------------------ */
int posfeat_sample_desc(const float *fmap, int b, int c, int h, int w, int cstride,
                        const float *coord, int npts, const int32_t *n_valid, int normalize,
                        float *out, void *stream);

/* posfeat_sample_desc with one valid-row count per image: n_valid[b] (device
 * int32, required), e.g. posfeat_detect_each's n_sel. */
int posfeat_sample_desc_each(const float *fmap, int b, int c, int h, int w, int cstride,
                             const float *coord, int npts, const int32_t *n_valid, int normalize,
                             float *out, void *stream);

/* NCHW <-> NHWC helpers used at the API boundary (torch tensors are NCHW). */
int posfeat_nchw_to_nhwc(const float *x, int n, int c, int h, int w, int cstride_out,
                         float *y, void *stream);
int posfeat_nhwc_to_nchw(const float *x, int n, int c, int h, int w, int cstride_in,
                         float *y, void *stream);

/* Extraction input on the device.  Replaces the per-image host transform of
 *   datasets/hpatches.py:14-17 / aachen.py / ETH_local_feature.py
 *   (transforms.ToTensor + Normalize(ImageNet mean/std)) so only the uint8
 *   image crosses PCIe: src uint8 [b][h][w][3] (row pitch src_pitch bytes),
 *   dst float [b][3][h][w] = ((u / 255) - mean) / std, bit-identical to the
 *   host's fp32 numpy/torch computation. */
int posfeat_normalize_rgb8(const unsigned char *src, int b, int h, int w, int src_pitch,
                           float *dst, void *stream);

/* ------------------------------------------------------------------------
 * Training-side dense correlation (forward values).
 * Replaces: losses/preprocess.py:27-121 Preprocess_Line2Window.forward with
 *   generate_kpts_regular_grid_random (preprocess_utils.py:598-659, identity
 *   map), epipolar_line_search (661-694, use_nn, loc_rand), get_endpoints
 *   (696-719), get_expected_correspondence_within_window (721-758); and
 *   losses/epipolarloss.py:38-101 EpipolarLoss_full.forward.
 * xf1/xf2: NHWC local maps [b][H/4][W/4] (128 channels, pixel stride cs).
 * F1/F2: [b][3][3].  sel1/sel2: [b][n] Categorical draw (0..grid^2-1) per
 * grid cell; rand1/rand2: [b][n][2] U(0,1) (loc_rand jitter).  The caller owns
 * the RNG; n = (H/grid)*(W/grid) per image (n1 for image 1, n2 for image 2).
 * Limits: H, W multiples of 4; 2 <= line_step <= 128 (POSFEAT_E_INVALID);
 * n2 % 4 == 0 and 1 <= (int)(window_size * H/4) * (int)(window_size * W/4) <=
 * 512 window taps per image with both factors >= 1 (POSFEAT_E_UNSUPPORTED).
 * Every refusal is made before any output is written.
 * Outputs (caller buffers, [b][n][...]):
 * ------------------------------------------------------------------------ */
typedef struct {
  float *coord1, *coord2;       /* grid points, pixels [b][n][2]             */
  float *g1, *g2;               /* feat{1,2}g_corloc, pixels                 */
  float *g1_std, *g2_std;       /* feat{1,2}g_std [b][n]                     */
  float *l1_exp_n, *l2_exp_n;   /* line expectation + jitter, normalised     */
  float *l1_org_n, *l2_org_n;   /* line expectation before jitter, normalised*/
  uint8_t *valid1, *valid2;     /* valid_epi{1,2}                            */
  float *w1, *w2;               /* feat{1,2}w_corloc, pixels                 */
  float *w1_std, *w2_std;       /* feat{1,2}w_std                            */
} posfeat_l2w_out;

size_t posfeat_line2window_workspace(int b, int H1, int W1, int H2, int W2, int grid);
int posfeat_line2window(const float *xf1, int cs1, const float *xf2, int cs2, int b, int H1,
                        int W1, int H2, int W2, const float *F1, const float *F2,
                        const int32_t *sel1, const int32_t *sel2, const float *rand1,
                        const float *rand2, float temperature, int grid, float window_size,
                        int line_step, posfeat_l2w_out *out, void *ws, size_t ws_bytes,
                        void *stream);
/* out[7] = {loss, loss_g1, loss_w1, loss_g2, loss_w2, percent_g, percent_w}.
 * n1 / n2: points per image of side 1 (c1, g1, w1, sg1, sw1, v1) and of side 2
 * (c2, g2, w2, sg2, sw2, v2); they differ when the two images differ in size.
 * Every mean is over its own side's b * n points. */
int posfeat_epipolar_loss(int b, int n1, int n2, const float *F1, const float *F2, const float *c1,
                          const float *c2, const float *g1, const float *g2, const float *w1,
                          const float *w2, const float *sg1, const float *sg2, const float *sw1,
                          const float *sw2, const uint8_t *v1, const uint8_t *v2,
                          float short_edge, float grid_thr, float win_thr, float weight_grid,
                          float weight_window, float *out, void *stream);

/* Backward of the descriptor loss (configs/train_desc.yaml: weight_grid 0,
 * weight_window 1, use_std_as_weight): dL/d local_map for both images, i.e.
 * what loss.backward() sends from losses/epipolarloss.py:38-101 through
 * losses/preprocess.py:98-101 (window expectation, preprocess_utils.py:
 * 721-758) and the query descriptors (sample_feat_by_coord, 40-53) into the
 * backbone (managers/trainer.py:331).  The std weights are detached
 * (epipolarloss.py:29-31) and the line search runs under no_grad
 * (preprocess_utils.py:661), so no other path carries gradient.
 * Call after posfeat_line2window on the SAME fwd_ws with its outputs `fwd`
 * (coord*, l*_exp_n, w*, w*_std, valid* are read).  dxf1/dxf2: NHWC
 * [b][H/4][W/4] (pixel stride dcs, 128 channels), overwritten.  Scatters
 * accumulate in 64-bit fixed point, so the result is deterministic.
 * Invariant the query-descriptor gradient relies on: fwd->coord1 / coord2
 * are the forward's own grid points, point i inside its own grid cell i =
 * cy (W / grid) + cx (n = (H / grid)(W / grid) points, one per cell, as
 * posfeat_line2window draws them): each map pixel gathers its gradient from
 * the cells whose sample can have it as a bilinear corner, so a point moved
 * outside its cell between the two calls would lose its gradient (the
 * descriptor-training step never edits them).
 * weight_grid != 0 returns POSFEAT_E_UNSUPPORTED. */
size_t posfeat_line2window_backward_workspace(int b, int H1, int W1, int H2, int W2, int grid);
int posfeat_line2window_backward(const float *xf1, int cs1, const float *xf2, int cs2, int b,
                                 int H1, int W1, int H2, int W2, const float *F1,
                                 const float *F2, const posfeat_l2w_out *fwd, const void *fwd_ws,
                                 float temperature, int grid, float window_size,
                                 float short_edge, float grid_thr, float win_thr,
                                 float weight_grid, float weight_window, float *dxf1, int dcs1,
                                 float *dxf2, int dcs2, void *ws, size_t ws_bytes, void *stream);

/* DiskLoss forward (losses/kploss.py:132-197, constant_reward, grid 8):
 * kp1/kp2 [b][H][W] score maps, xf1/xf2 NHWC local maps [b][H/4][W/4] (pixel
 * stride cs), F1/F2 [b][3][3].  Either prop1,prop2,acc1,acc2 ([b][n] Categorical proposal
 * 0..63 and Bernoulli acceptance) are given, or uni1/uni2 ([b][n][65] U(0,1):
 * 64 Gumbel-max uniforms + 1 acceptance uniform) and the kernel samples.
 * out[4] = {loss, reinforce, kp_penalty, n_kps}. */
size_t posfeat_disk_loss_workspace(int b, int H, int W);
int posfeat_disk_loss(const float *kp1, const float *kp2, const float *xf1, int cs1,
                      const float *xf2, int cs2, int b, int H, int W, const float *F1,
                      const float *F2, const int32_t *prop1, const int32_t *prop2,
                      const uint8_t *acc1, const uint8_t *acc2, const float *uni1,
                      const float *uni2, float temperature, float reward_thr, float good_reward,
                      float bad_reward, float kp_penalty, float *out, void *ws, size_t ws_bytes,
                      void *stream);

/* DiskLoss forward + gradient w.r.t. both score maps (the backward of
 * losses/kploss.py:132-197 with cor_detach=True, match_grad=False as in
 * configs/train_kp.yaml:69-73: only the keypoint log-probabilities of
 * point_distribution (20-35) carry gradient).  Same arguments as
 * posfeat_disk_loss plus dkp1/dkp2 [b][H][W] (overwritten). */
size_t posfeat_disk_loss_grad_workspace(int b, int H, int W);
int posfeat_disk_loss_grad(const float *kp1, const float *kp2, const float *xf1, int cs1,
                           const float *xf2, int cs2, int b, int H, int W, const float *F1,
                           const float *F2, const int32_t *prop1, const int32_t *prop2,
                           const uint8_t *acc1, const uint8_t *acc2, const float *uni1,
                           const float *uni2, float temperature, float reward_thr,
                           float good_reward, float bad_reward, float kp_penalty, float *out,
                           float *dkp1, float *dkp2, void *ws, size_t ws_bytes, void *stream);

/* Weight gradient of a stride-1 "same" conv (the autograd conv2d weight/bias
 * backward behind managers/trainer.py:331): dw [cout][Kpad] in the packed K
 * order of posfeat_conv2d_nhwc (so it lines up with the packed weights),
 * db [cout] (may be NULL).  dy: NHWC [n][h][w] pitch dy_cstride; x: NHWC
 * input pitch x_cstride; cin % 32 == 0 or cin == 4; cout % 32 == 0; odd
 * square kernel.  Deterministic (pixel-split partials summed in order). */
size_t posfeat_conv_wgrad_workspace(int n, int h, int w, int cin, int cout, int kh, int kw);
int posfeat_conv_wgrad(const float *dy, int dy_cstride, const float *x, int x_cstride, int n,
                       int h, int w, int cin, int cout, int kh, int kw, float *dw, float *db,
                       void *ws, size_t ws_bytes, void *stream);

/* Winograd 3x3 stride-1 pad-1 conv (the decoder layers,
 * networks/DescNet.py:41-45, as the engine runs them): F(4x4,3x3) when h and w
 * are multiples of 4 (36 transformed weight matrices), else F(2x2,3x3) (16).
 * U ([36][cout][cin] floats) from the engine-packed weights by
 * posfeat_wino_weights for the same (h, w); then input transform -> the
 * transform-domain GEMMs (one launch) -> output transform + bias + act into y
 * (pixel stride y_cstride).  h, w even; cin % 32 == 0.  Same result as
 * posfeat_conv2d_nhwc within fp32 rounding (transform-grown). */
size_t posfeat_wino_workspace(int n, int h, int w, int cin, int cout);
int posfeat_wino_weights(const float *w_packed, int cout, int cin, int h, int w, float *U,
                         void *stream);
int posfeat_conv3x3_wino(const float *x, int x_cstride, int n, int h, int w, int cin,
                         const float *U, const float *bias, int cout, int act, float *y,
                         int y_cstride, void *ws, size_t ws_bytes, void *stream);

/* The same conv by Winograd F(6x6,3x3) (the extraction engine's decoder and
 * head.conv1, networks/DescNet.py:41-45 and DeteNet.py:102-121): 64
 * transformed weight matrices U ([64][cout][cin] floats, posfeat_wino6_weights),
 * 6x6 output tiles (the last tile row / column cut at h, w), 1.27x fewer
 * transform-domain MACs than F(4x4).  Any h, w; cin % 32 == 0, cout % 4 == 0,
 * even pitches.  Same result as posfeat_conv2d_nhwc within fp32 rounding
 * grown by the transforms (B^T, A^T exact; G in ninths). */
size_t posfeat_wino6_workspace(int n, int h, int w, int cin, int cout);
int posfeat_wino6_weights(const float *w_packed, int cout, int cin, float *U, void *stream);
int posfeat_conv3x3_wino6(const float *x, int x_cstride, int n, int h, int w, int cin,
                          const float *U, const float *bias, int cout, int act, float *y,
                          int y_cstride, void *ws, size_t ws_bytes, void *stream);
/* The engine's variants of the same conv: planes = 1 -- U as three bf16
 * planes (96 x cout x cin halves, posfeat_wino6_weights_planes; cout % 64 ==
 * 0), the GEMM splitting V on the fly (bf16x6); up2 = 1 -- x is the (h/2, w/2)
 * map and the conv reads its x2 bilinear upsample (align_corners = True,
 * DescNet.py:182-190 upconv), formed inside the input transform (h, w even).
 * posfeat_wino6_weights_floats: the U size in floats for those arguments. */
size_t posfeat_wino6_weights_floats(int cin, int cout, int planes);
int posfeat_wino6_weights_planes(const float *w_packed, int cout, int cin, int planes, float *U,
                                 void *stream);
int posfeat_conv3x3_wino6_ex(const float *x, int x_cstride, int n, int h, int w, int cin,
                             const float *U, int planes, int up2, const float *bias, int cout,
                             int act, float *y, int y_cstride, void *ws, size_t ws_bytes,
                             void *stream);
/* Weight gradient of the same conv by F(6x6) (the training step's decoder,
 * behind managers/trainer.py:331): dM = A dY A^T, 64 transform-domain GEMMs,
 * dw = G^T dU G in the packed K order; db (may be NULL) = sum of dy.  Any h,
 * w; cin, cout % 128 == 0.  Deterministic. */
size_t posfeat_wino6_wgrad_workspace(int n, int h, int w, int cin, int cout);
int posfeat_conv3x3_wino6_wgrad(const float *dy, int dy_cstride, const float *x, int x_cstride,
                                int n, int h, int w, int cin, int cout, float *dw, float *db,
                                void *ws, size_t ws_bytes, void *stream);

/* Weight gradient of the same decoder convs by F(4x4,3x3) (the autograd
 * conv2d weight/bias backward behind managers/trainer.py:331 for
 * networks/DescNet.py:41-45): dM = A dY A^T per 4x4 output tile, the 36
 * transform-domain GEMMs dU_xi = sum_tiles dM_xi (x) V_xi (one launch, split
 * over tiles), dw = G^T dU G written in the packed K order of
 * posfeat_conv2d_nhwc; db (may be NULL) = sum of dy.  h, w % 4 == 0;
 * cin, cout % 128 == 0.  Deterministic. */
size_t posfeat_wino_wgrad_workspace(int n, int h, int w, int cin, int cout);
int posfeat_conv3x3_wino_wgrad(const float *dy, int dy_cstride, const float *x, int x_cstride,
                               int n, int h, int w, int cin, int cout, float *dw, float *db,
                               void *ws, size_t ws_bytes, void *stream);

/* torch.optim.SGD step without momentum/weight decay (train_kp.yaml:11-13,
 * managers/trainer.py:118-119, 356): w -= lr * g over n floats. */
int posfeat_sgd(float *w, const float *g, long long n, float lr, void *stream);

/* ------------------------------------------------------------------------
 * Whole-model extraction engine.
 * Replaces: networks/PoSFeat_model.py:91-134 PoSFeat.extract for the
 *   effective model ResUNet(resnet50, 128/128) + KeypointDet(192, 1,
 *   'identity', 'Softplus') (configs/train_desc.yaml:16-31), i.e.
 *   networks/DescNet.py:64-84 and networks/DeteNet.py:102-121.
 * Weights: one packed fp32 blob; layer i occupies w_off/b_off floats (from
 *   posfeat_model_conv_spec).  The spec named "head.prelu" holds the shared
 *   PReLU scalar at b_off.
 * ------------------------------------------------------------------------ */
typedef struct posfeat_model posfeat_model;

typedef struct {
  float *local_map;       /* [b][128][h/4][w/4]  NCHW (may be NULL)        */
  float *global_map;      /* [b][128][h/16][w/16] NCHW (may be NULL)       */
  float *global_feat;     /* [b][128]                 (may be NULL)        */
  float *local_point;     /* [b][1][h][w]                                  */
  float *local_map_small; /* [b][64][h/4][w/4]  NCHW (may be NULL)         */
  const float *local_map_nhwc; /* OUT: engine-internal NHWC local_map     */
  int local_map_cstride;       /* OUT: its pixel stride in floats          */
} posfeat_extract_out;

int posfeat_model_num_specs(void);
int posfeat_model_conv_spec(int i, const char **name, int *cout, int *cin, int *kh, int *kw,
                            long long *w_off, long long *b_off);
long long posfeat_model_weight_floats(void);
int posfeat_model_create(int batch, int h, int w, const float *weights, posfeat_model **out);
/* The same, sharing the derived-weight store of `share` (an extraction
 * instance made from the same `weights` pointer; NULL: a store of its own):
 * the blob's bf16 planes and the Winograd-domain weights (F(4x4) and F(2x2)
 * slots) are built once for every instance of an engine, whatever image
 * sizes they serve, and destroying one instance frees no device memory while
 * another still uses the store (Extractor over many image sizes,
 * managers/extractor.py:357-382 with datasets/hpatches.py:35-38's crops).
 * Instances sharing a store may run on different streams: a forward orders
 * itself after the forward that last built derived weights.  They also share
 * one side stream and its fork / join events (KeypointDet's image branch):
 * instances sharing a store must be driven from ONE host thread (their
 * forwards then serialise on that side stream, as the Extractor's loop
 * does); give concurrent host threads separate stores (share = NULL). */
int posfeat_model_create_shared(int batch, int h, int w, const float *weights,
                                posfeat_model *share, posfeat_model **out);
/* An extraction instance (posfeat_model_create) builds its derived weights --
 * the blob's bf16 planes and the Winograd-domain weights -- once, in device
 * memory of its store (allocated by its first forward), by the first forward
 * that needs them.  A caller that rewrites the weight blob in place calls
 * this before the next forward: every instance sharing the store rebuilds
 * (training instances rebuild them every forward and ignore it). */
int posfeat_model_weights_changed(posfeat_model *m);
size_t posfeat_model_workspace(const posfeat_model *m);
/* The process-wide conv tile choices (the engine's autotuner: tiles never
 * change results, only speed) as text, one "<descriptor class>|<n>/<h>/<w>
 * <tile>" line each: export writes them into buf (cap bytes; *len = bytes
 * needed incl. the NUL; buf NULL: size query), import adds lines not yet
 * known and returns how many.  A tuning database kept between processes
 * (records/tile_db.txt): a new image size within 25 % of a stored GEMM M
 * reuses its tile instead of timing every candidate. */
int posfeat_tile_cache_export(char *buf, size_t cap, size_t *len);
int posfeat_tile_cache_import(const char *text);
int posfeat_model_extract(posfeat_model *m, const float *img_nchw, posfeat_extract_out *out,
                          void *ws, size_t ws_bytes, void *stream);
/* ResUNet.forward alone (networks/DescNet.py:64-84): fills out->local_map,
 * global_map, local_map_small (and global_feat) when non-NULL; local_point is
 * not touched.  Eval-mode BatchNorm (folded), as PoSFeat.extract uses it. */
int posfeat_model_backbone(posfeat_model *m, const float *img_nchw, posfeat_extract_out *out,
                           void *ws, size_t ws_bytes, void *stream);
/* KeypointDet.forward([x, img]) alone (networks/DeteNet.py:102-121):
 * x_nchw = cat[local_map, local_map_small] [b][192][h/4][w/4] (the input
 * PoSFeat.extract builds, PoSFeat_model.py:97-102), img_nchw [b][3][h][w];
 * writes local_point [b][1][h][w]. */
int posfeat_model_keypointdet(posfeat_model *m, const float *x_nchw, const float *img_nchw,
                              float *local_point, void *ws, size_t ws_bytes, void *stream);
/* Optional per-kernel timing: when enabled, extract() records hipEvents
 * around every launch; posfeat_model_timing() returns the summed ms of the
 * last call for launches whose label starts with `prefix`. */
int posfeat_model_set_timing(posfeat_model *m, int enable);
int posfeat_model_timing(posfeat_model *m, const char *prefix, double *ms, double *flops,
                         int *launches);
/* The i-th timed launch of the last call (diagnostic; host-synchronises):
 * its label (valid until the next call on m), duration and the FLOPs the
 * engine counts for it.  POSFEAT_E_INVALID past the last launch. */
int posfeat_model_timing_event(posfeat_model *m, int i, const char **label, double *ms,
                               double *flops);
/* the arithmetic of the i-th timed label's MFMA launches: a mask of 1 (fp32
 * MFMA) and 2 (bf16x6, fp32-exact products on the bf16 matrix cores); 0 for a
 * label without MFMA work.  Diagnostics for bench.py's rooflines (no
 * reference counterpart). */
int posfeat_model_timing_event_arith(posfeat_model *m, int i);
void posfeat_model_destroy(posfeat_model *m);

/* Keypoint-head training (config 5, configs/train_kp.yaml: optimal_modules
 * ['localheader'], backbone frozen and detached, PoSFeat_model.py:97-102).
 * A model made by posfeat_model_create_train keeps in its workspace what the
 * backward needs (it materialises head.conv2's input instead of the phase
 * path; results identical within fp32 rounding).
 * posfeat_model_head_backward: given dL/d local_point [b][h][w] of the LAST
 * extract() on the same workspace, writes dL/d(head parameters) into grad
 * (posfeat_model_head_floats() floats, laid out exactly like the weight blob
 * from float posfeat_model_head_offset() on: conv1, convimg, conv2, conv3,
 * prelu).  Replaces the autograd backward of networks/DeteNet.py:102-121
 * (managers/trainer.py:330-331). */
int posfeat_model_create_train(int batch, int h, int w, const float *weights,
                               posfeat_model **out);
long long posfeat_model_head_offset(void);
long long posfeat_model_head_floats(void);
int posfeat_model_head_backward(posfeat_model *m, const float *dlocal_point, float *grad,
                                void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Descriptor training (config 3, configs/train_desc.yaml: optimal_modules
 * ['backbone'], Adam lr 1e-4).  Train-mode ResUNet (BatchNorm with batch
 * statistics and running-stat update) forward and backward.
 * Replaces: the autograd forward/backward of networks/DescNet.py:64-84 under
 *   backbone.train() (managers/trainer.py:293-297, 330-331) and
 *   torch.optim.Adam.step (trainer.py:118-119, 356).
 * Layout: one packed fp32 parameter blob (per layer: conv weight [cout][Kpad]
 *   as the engine packs it, conv bias when the layer has one, BN weight, BN
 *   bias -- offsets from posfeat_bbtrain_layer offs[0..3]); the gradient blob
 *   has the same layout; running mean / var live in a second blob
 *   (offs[4], offs[5]).  Layer names follow posfeat_model_conv_spec.
 * Workspaces: forward() fills `act` (posfeat_bbtrain_act_bytes, one per image
 *   batch: im1 and im2 keep separate BN statistics, PoSFeat_model.py:144-145);
 *   backward() reads the same `act`; `scratch` is shared.  All 256-B aligned.
 * forward: img [b][3][h][w] NCHW; *local_map_nhwc = the NHWC local map
 *   [b][h/4][w/4][128] inside `act`.  stats may be NULL (no running update).
 * backward: dlocal_map NHWC (pixel stride dcs); grad = (accumulate ? grad : 0)
 *   + dL/d params.  h and w must be multiples of 16.  An accumulate = 0 call
 *   derives every layer's input-gradient weights (transposed / phase weights,
 *   their bf16 planes, the Winograd U) into `scratch`; an accumulate = 1 call
 *   reuses them, so it must follow an accumulate = 0 call with the SAME params
 *   and scratch (the second image batch of one step, as the trainer does).
 * posfeat_adam: torch.optim.Adam (no amsgrad) on n floats; g is scaled by
 *   grad_scale first (1/world after a summing all-reduce = DDP's mean). */
typedef struct posfeat_bbtrain posfeat_bbtrain;

/* SyncBatchNorm groups (group.hip).  Replaces the SyncBatchNorm conversion of
 *   networks/PoSFeat_model.py:48-55 (PoSFeat.set_parallel): with a group set
 *   (posfeat_bbtrain_set_group), every BatchNorm of the train-mode backbone
 *   sums its statistics over the group's ranks -- forward (sum y, sum y^2,
 *   count) and backward (sum g, sum g x^) -- as torch's SyncBatchNorm does;
 *   dgamma / dbeta stay per rank (DDP averages them with the other grads).
 * RCCL: rank 0 calls posfeat_group_unique_id (128 bytes), the host broadcasts
 *   them (torch.distributed), every rank calls posfeat_group_create_rccl.
 * local: `world` ranks that are threads of one process on one device (the
 *   one-GPU test of the cross-rank semantics).
 * host: a process group without RCCL (torch.distributed over gloo, e.g. ranks
 *   that share one device): each exchange copies the n doubles to the host
 *   (the stream is synchronised), calls allreduce(buf, n, user) -- which must
 *   sum buf in place over the ranks and return 0 -- and copies them back. */
typedef struct posfeat_group posfeat_group;
typedef struct posfeat_local_group posfeat_local_group;
typedef int (*posfeat_host_allreduce_fn)(double *buf, int n, void *user);
int posfeat_group_unique_id(void *out128);
int posfeat_group_create_rccl(int world, int rank, const void *id128, posfeat_group **out);
int posfeat_group_create_host(int world, int rank, posfeat_host_allreduce_fn allreduce,
                              void *user, posfeat_group **out);
int posfeat_local_group_create(int world, int max_doubles, posfeat_local_group **out);
int posfeat_group_create_local(posfeat_local_group *L, int rank, posfeat_group **out);
void posfeat_group_destroy(posfeat_group *g);
void posfeat_local_group_destroy(posfeat_local_group *L);
int posfeat_bbtrain_set_group(posfeat_bbtrain *m, posfeat_group *g);
int posfeat_bbtrain_num_layers(void);
int posfeat_bbtrain_layer(int i, const char **name, int *cin, int *cout, int *k, int *stride,
                          int *has_bias, long long *offs /* [6] */);
long long posfeat_bbtrain_param_floats(void);
long long posfeat_bbtrain_stat_floats(void);
int posfeat_bbtrain_create(int batch, int h, int w, posfeat_bbtrain **out);
size_t posfeat_bbtrain_act_bytes(const posfeat_bbtrain *m);
size_t posfeat_bbtrain_scratch_bytes(const posfeat_bbtrain *m);
int posfeat_bbtrain_forward(posfeat_bbtrain *m, const float *params, float *stats, float momentum,
                            const float *img_nchw, void *act, void *scratch,
                            float **local_map_nhwc, void *stream);
int posfeat_bbtrain_backward(posfeat_bbtrain *m, const float *params, const void *act,
                             const float *dlocal_map_nhwc, int dcs, float *grad, int accumulate,
                             void *scratch, void *stream);
int posfeat_bbtrain_set_timing(posfeat_bbtrain *m, int enable);
int posfeat_bbtrain_timing(posfeat_bbtrain *m, const char *prefix, double *ms, double *flops,
                           int *launches);
/* The i-th timed launch of the last timed step (labels "fwd:conv:<layer>",
 * "bwd:wgrad:<layer>", "bwd:dgrad:<layer>", "fwd:bn", ...): label, ms, flops;
 * POSFEAT_E_INVALID past the last.  Host-synchronises. */
int posfeat_bbtrain_timing_event(posfeat_bbtrain *m, int i, const char **label, double *ms,
                                 double *flops);
/* as posfeat_model_timing_event_arith, for the training step's labels */
int posfeat_bbtrain_timing_event_arith(posfeat_bbtrain *m, int i);
void posfeat_bbtrain_destroy(posfeat_bbtrain *m);
int posfeat_adam(float *p, const float *g, float *m, float *v, long long n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, long long step, float grad_scale,
                 void *stream);

/* DiskLoss's flash LSE pass alone (kploss.py:160-166: the normaliser of
 * Categorical(logits=affinity)): lse[b][j] = logsumexp_i(T <fa_i, fb_j> - T) over
 * the n rows of fa for each row j of fb, fa/fb [b][n][128]; the n x n
 * similarity is recomputed by fp32 MFMA and never stored. */
size_t posfeat_disk_flash_lse_workspace(int b, int n);
int posfeat_disk_flash_lse(const float *fa, const float *fb, int b, int n, float T, float *lse,
                           void *ws, size_t ws_bytes, void *stream);
/* The launch plan of the flash passes for b pairs of n points (host only, no
 * device needed): the number of A-row splits and the rows each owns, as
 * posfeat_disk_loss[_grad] (n = (H / 8)(W / 8)) and posfeat_disk_flash_lse
 * launch them.  Split s covers rows [s * rows_per_split, (s + 1) *
 * rows_per_split) of all n points in the LSE passes and of the accepted
 * points in the SUM passes. */
int posfeat_disk_flash_plan(int b, int n, int *nsplit, int *rows_per_split);

/* ---- evaluation matchers ---------------------------------
 * Replaces mnn_matcher (losses/preprocess_utils.py:795-803 =
 * evaluations/hpatches/evaluation.py:28-38), mutual_nn_matcher / ratio_matcher /
 * mutual_nn_ratio_matcher (evaluations/aachen/matchers.py:5-75, the same code
 * as evaluations/ETH_local_feature/custom_matcher.py) for L2-normalised
 * descriptors d1 [n1][dim], d2 [n2][dim] (dim == 128, 16-B aligned).
 * mode: 0 mutual NN, 1 symmetric Lowe ratio, 2 mutual NN + ratio.
 * matches: int32 [n1][2] capacity, written in ascending first index;
 * *count (device) = number written.  Tie rule: the first (lowest) index wins
 * an arg-max tie; the second-best similarity is the 2nd largest value with
 * multiplicity (torch.topk(2)).  sim = d1 d2^T is never materialised. */
size_t posfeat_match_workspace(int n1, int n2);
int posfeat_match(const float *d1, int n1, const float *d2, int n2, int dim, int mode, float ratio,
                  int32_t *matches, int32_t *count, void *ws, size_t ws_bytes, void *stream);

/* ---- batched pair-list matching and the HPatches reprojection check -------
 * posfeat_match over a whole pair list in four launches (one top-2 launch
 * over a flat tile list covering both sides of every pair, one merge, one
 * select with a workgroup per pair, after one plan upload), for the loops of
 * evaluations/hpatches/evaluation.py:49-67 (image 1 against images 2..6 of
 * every sequence) and evaluations/aachen/reconstruct_pipeline.py
 * match_features (one matcher call per listed pair).
 *
 * desc [N][dim] is one pool of descriptors (dim == 128, 16-B aligned); set s
 * is its rows [set_off[s], set_off[s+1]).  set_off (nsets + 1 entries) and
 * pairs (npairs x (s1, s2)) are HOST arrays; pairs may share sets on either
 * side.  Pair p writes its matches at row moff[p] = sum_{q<p} n1(q) of
 * matches [sum n1][2], ascending in the first index, with the set-local
 * indices, mode, ratio arithmetic and tie rule of posfeat_match (the
 * similarity bits do not depend on how the plan splits the rows, so the
 * output equals posfeat_match's on that pair alone); counts[p] (device) = rows
 * written; a pair with an empty side gives counts[p] = 0.
 * Returns, before any device work: POSFEAT_E_INVALID for a null pointer, a
 * set index out of range, a negative or decreasing set_off, or sum n1 past
 * INT32_MAX; POSFEAT_E_UNSUPPORTED for dim != 128 or mode outside 0..2;
 * POSFEAT_E_WORKSPACE for ws_bytes below posfeat_match_pairs_workspace (0 for
 * an invalid table).  ws must be 256-B aligned.
 * Stream-ordered, never waits for its own kernels; NOT graph-capturable: the
 * call copies its plan (side and tile tables) from pageable host memory into
 * ws, a copy the runtime may carry out before it returns.
 * posfeat_match_pairs_splits (host only) reports the plan: nsplit[2p] and
 * nsplit[2p+1] = the number of row ranges the d2 rows (side "rows of sim")
 * and the d1 rows (side "columns") of pair p are cut into; 0 for a pair with
 * an empty side. */
size_t posfeat_match_pairs_workspace(const int32_t *set_off, int nsets, const int32_t *pairs,
                                     int npairs);
int posfeat_match_pairs_splits(const int32_t *set_off, int nsets, const int32_t *pairs, int npairs,
                               int32_t *nsplit);
int posfeat_match_pairs(const float *desc, const int32_t *set_off, int nsets, const int32_t *pairs,
                        int npairs, int dim, int mode, float ratio, int32_t *matches,
                        int32_t *counts, void *ws, size_t ws_bytes, void *stream);

/* Guided matching: posfeat_match_pairs with the candidates of every pair
 * restricted by the pair's verified two-view model (what COLMAP's guided
 * matching does after two-view geometry; the reference hands this to COLMAP).
 * desc, set_off, nsets, pairs, npairs, dim, mode, ratio, matches, counts, ws
 * and stream mean what they mean for posfeat_match_pairs; the tile plan
 * (posfeat_match_pairs_splits), the output layout and the tie rule are that
 * call's.  In addition: kp [N][2] fp32 keypoints (x, y), pool rows numbered as
 * desc; model: 0 homography, 1 fundamental matrix; M [npairs][9] fp64
 * row-major (device, 8-B aligned): what posfeat_ransac_homography /
 * posfeat_ransac_fundamental write, used as given, never rescaled; thr in
 * pixels, t2 = (float)(thr * thr).  Conventions of posfeat_ransac_fundamental:
 * x1 = (x, y, 1) in image 1 (set s1), x2 = (u, v, 1) in image 2, x2^T F x1 =
 * 0, x2 ~ H x1.  A descriptor of one image competes only against the keypoints
 * of the other image the model admits: arg-max, second best and Lowe ratio are
 * all taken over the admissible set.  No arithmetic below is contracted, each
 * operation is rounded once.
 *   records      one fp32 x 4 record per keypoint of the pair's two images,
 *                built in fp64 by a prepass launch.  For a point (a, b) and a
 *                matrix Q, q_k = (Q[k][0] a + Q[k][1] b) + Q[k][2], k = 0..2.
 *                Fundamental: rec1[i] = (q0, q1, q2, q0 q0 + q1 q1) with Q = F
 *                for image-1 point i, rec2[j] the same with Q = F^T for image-2
 *                point j, each component rounded to fp32 last.  Homography:
 *                rec1[i] = (q0 / q2, q1 / q2, 0, 0) with Q = H, rounded to fp32
 *                last, no sign test on q2; rec2[j] = (u, v, 0, 0).
 *   admissible   in fp32, inside the top-2 fold, from the streamed row's
 *                record ra and the column's data.  Fundamental, side "rows of
 *                sim" (streamed rows image 2, columns image 1): e = ((ra0 x) +
 *                (ra1 y)) + ra2 with (x, y) the column's fp32 keypoint, den = ra3
 *                + rec1[col].w; side "columns": the same with rec1 streamed, (u,
 *                v) and rec2[col].w; both: admissible iff den > 0 and t2 den is
 *                finite and e e <= t2 den.  Homography (either side): du = u -
 *                px, dv = v - py with (px, py) from rec1 and (u, v) from rec2,
 *                admissible iff (du du + dv dv) <= t2.  Any NaN fails.  A zero
 *                model (status 1 from RANSAC) admits nothing: counts[p] = 0.
 *                The two sides of a fundamental pair evaluate e from different
 *                records and may disagree at the threshold; that is part of
 *                the definition (a mutual match needs both).
 *   fold         an inadmissible entry takes -inf, as a row past the range
 *                does; the K = 128 chain, the k order and the strict '>' are
 *                posfeat_match's.
 *   select       posfeat_match's, plus: a row whose best value is -inf (no
 *                admissible candidate) never matches, in any mode.  A row with a
 *                single admissible candidate has second best -inf; its ratio is
 *                d1 / (inf + 1e-8) = 0, which passes every ratio test.
 * Returns, before any device work: posfeat_match_pairs's errors;
 * POSFEAT_E_INVALID for a null kp or M, an M not 8-B aligned, a non-finite or
 * non-positive thr; POSFEAT_E_UNSUPPORTED for a model outside 0..1;
 * POSFEAT_E_WORKSPACE for ws_bytes below posfeat_match_pairs_guided_workspace
 * (the unguided workspace plus a pair table and 16 B per keypoint per pair
 * side; 0 for an invalid table).
 * Launches: the record prepass, top-2, merge (only when a side is split),
 * select.  Stream-ordered, never waits for its own kernels; NOT
 * graph-capturable (the plan is copied from pageable host memory).
 * Deterministic, and a pair's result does not depend on the rest of the list.
 * posfeat_guided_record and posfeat_guided_admissible are host only (no
 * device, no launch) and compile the text the kernels compile.
 * posfeat_guided_record writes to rec[4] the record of the point pt[2] under
 * M[9]: side 0 an image-1 point (rec1), side 1 an image-2 point (rec2).
 * posfeat_guided_admissible returns 1 or 0 for a streamed record ra[4] and the
 * column's data col[3]: fundamental (x, y, w) = the column's keypoint and the w
 * of its record; homography (x, y, unused) = the column's record.  Both return
 * POSFEAT_E_INVALID for a null pointer (a side outside 0..1, a non-finite or
 * non-positive thr) and POSFEAT_E_UNSUPPORTED for a model outside 0..1. */
size_t posfeat_match_pairs_guided_workspace(const int32_t *set_off, int nsets,
                                            const int32_t *pairs, int npairs);
int posfeat_guided_record(int model, int side, const double *M, const float *pt, float *rec);
int posfeat_guided_admissible(int model, const float *ra, const float *col, double thr);
int posfeat_match_pairs_guided(const float *desc, const float *kp, const int32_t *set_off,
                               int nsets, const int32_t *pairs, int npairs, int dim, int mode,
                               float ratio, int model, const double *M, double thr,
                               int32_t *matches, int32_t *counts, void *ws, size_t ws_bytes,
                               void *stream);

/* The homography check of evaluations/hpatches/evaluation.py:69-90 on the
 * matches posfeat_match_pairs left: kp [N][2] fp32 keypoints (x, y) with the
 * row numbering of desc, set_off / pairs the same host tables, H [npairs][9]
 * fp64 row-major homographies (device).  Per match (a, b) of pair p, in fp64:
 * project (x_a, y_a, 1) by H[p], divide by the third component, take the
 * Euclidean distance to (x_b, y_b); hist[p][t-1] (int32 [npairs][nthr],
 * device) = the number of matches with dist <= t for t = 1..nthr
 * (1 <= nthr <= 32, else POSFEAT_E_INVALID).  NaN / inf distances count
 * nowhere; a pair without matches gives zeros.  ws: 256-B aligned,
 * posfeat_reproj_hist_workspace(npairs) bytes (the per-pair offsets, copied
 * from host memory: stream-ordered, no host synchronisation, not
 * graph-capturable). */
size_t posfeat_reproj_hist_workspace(int npairs);
int posfeat_reproj_hist(const float *kp, const int32_t *set_off, int nsets, const int32_t *pairs,
                        int npairs, const int32_t *matches, const int32_t *counts,
                        const double *H, int nthr, int32_t *hist, void *ws, size_t ws_bytes,
                        void *stream);

/* RANSAC homographies for every pair of a list, on the matches
 * posfeat_match_pairs left (no reference counterpart: the consumers of the
 * reference's matches call OpenCV on the host, one pair at a time).  kp,
 * set_off, pairs, matches and counts mean what they mean for
 * posfeat_reproj_hist.  Per pair p (its position in `pairs`), with n =
 * counts[p] matches, all in fp64:
 *   sampler      iteration `it` draws the four distinct match indices
 *                posfeat_ransac_sample(seed, p, it, n) gives: with mix() the
 *                splitmix64 finaliser, r = mix(mix(mix(seed ^ mix(p)) ^ it) ^ k),
 *                j = ((r >> 32) (n - k)) >> 32, then ++j for every earlier draw
 *                <= j taken in ascending order (k = 0..3);
 *   degeneracy   for each of the four point triples (i, j, k) of the sample, in
 *                each image, in pixels: cr = (pj - pi) x (pk - pi); the sample
 *                is rejected when |cr| <= 1e-6 |pj - pi| |pk - pi| or the sign
 *                of cr differs between the images;
 *   solve        the 8x8 system for h11..h32 (h33 = 1) in coordinates
 *                normalised per pair and per side over all its matches
 *                (centroid 0, mean distance sqrt 2), Gaussian elimination with
 *                partial pivoting, a pivot below 1e-12 times the largest entry
 *                of its column rejecting the sample; H = T2^-1 Hn T1;
 *   score        the residual of posfeat_reproj_hist: a match is an inlier iff
 *                its distance is finite and <= thr;
 *   selection    most inliers, ties to the lowest iteration; rejected samples
 *                never win;
 *   refit        least squares over the winner's inliers (same parametrisation
 *                and coordinates, normal equations accumulated in a fixed
 *                order), kept iff its inlier count is >= the winner's.
 * Outputs (device): H [npairs][9] row-major, Frobenius norm 1, H[8] >= 0;
 * info [npairs][4] = {status, n_inliers, best_iter, refit_kept}; inlier
 * [sum n1] uint8: inlier[moff[p] + i] = 1 iff match i < counts[p] of pair p is
 * an inlier of H[p], the pair's other rows 0.  status 1 (fewer than 4 matches,
 * or every sample rejected): H[p] = 0, n_inliers 0, best_iter -1, mask 0.  A
 * match with an index outside its set is never an inlier and takes no part in
 * the normalisation.
 * Returns, before any device work: POSFEAT_E_INVALID for a null pointer, a set
 * index out of range, a negative or decreasing set_off, sum n1 past INT32_MAX,
 * iters outside 1..65536, a non-finite or non-positive thr;
 * POSFEAT_E_WORKSPACE for ws_bytes below posfeat_ransac_homography_workspace
 * (0 for an invalid table or iteration count).  ws must be 256-B aligned.
 * Three launches whatever npairs; stream-ordered, never synchronises the host;
 * NOT graph-capturable (the pair table is copied from pageable host memory).
 * Deterministic: the same inputs give the same bits, and the result for a
 * pair index does not depend on the other pairs of the list.
 * posfeat_ransac_sample is host only (no device, no launch): the sampler the
 * kernels call; POSFEAT_E_INVALID for n < 4. */
int posfeat_ransac_sample(uint64_t seed, int pair, int iter, int n, int32_t out4[4]);
size_t posfeat_ransac_homography_workspace(const int32_t *set_off, int nsets,
                                           const int32_t *pairs, int npairs, int iters);
int posfeat_ransac_homography(const float *kp, const int32_t *set_off, int nsets,
                              const int32_t *pairs, int npairs, const int32_t *matches,
                              const int32_t *counts, int iters, double thr, uint64_t seed,
                              double *H, int32_t *info, uint8_t *inlier, void *ws,
                              size_t ws_bytes, void *stream);

/* RANSAC fundamental matrices for every pair of a list: the two-view
 * geometric verification the reference's Aachen and ETH pipelines hand to
 * COLMAP (evaluations/aachen/reconstruct_pipeline.py:224-231), on the matches
 * posfeat_match_pairs left.  kp, set_off, pairs, matches, counts, iters, thr,
 * seed, ws and stream mean what they mean for posfeat_ransac_homography.  Per
 * pair p with n = counts[p] matches, all in fp64, x1 = (x, y, 1) the image-1
 * point and x2 = (u, v, 1) the image-2 point of a match:
 *   sampler      iteration `it` draws the seven distinct match indices
 *                posfeat_ransac_sample_k(seed, p, it, n, 7, out) gives: the scheme
 *                of posfeat_ransac_sample continued to k = 0..6 (same mix, same
 *                base, ++j for every earlier draw <= j taken in ascending
 *                order), so its first four draws are that call's.  A sample
 *                holding a match with an index outside its set is rejected;
 *   coordinates  per pair and per side Ti = [s 0 -s cx; 0 s -s cy; 0 0 1]:
 *                centroid 0, mean distance sqrt 2 over all matches whose
 *                indices are inside their sets (posfeat_ransac_homography's);
 *   system       row i of the 7x9 system A f = 0 is (u x, u y, u, v x, v y, v,
 *                x, y, 1) of sample match i in normalised coordinates, f = Fn
 *                row-major (x2^T Fn x1 = 0);
 *   null space   Gaussian elimination with full pivoting: step s = 0..6 takes
 *                the largest |A[r][c]| over r >= s, c >= s (the first in
 *                row-major order on a tie), swaps it to (s, s) by a row and a
 *                column swap, and subtracts A[r][s] / A[s][s] times row s from
 *                every row r > s.  The sample is rejected when a pivot is below
 *                1e-12 times the largest |entry| of the system as given, or is
 *                not a positive number (a null space of more than two
 *                dimensions, e.g. a repeated match).  The two columns left at
 *                positions 7 and 8 are free: f1 has z = (1, 0) there, f2 has
 *                z = (0, -1), the other entries by back substitution (z[c] =
 *                -(A[c][7] z[7] + A[c][8] z[8] + sum_{c<k<7} A[c][k] z[k]) /
 *                A[c][c], c = 6..0), then the column swaps undone.  No entry of
 *                F is fixed, so F33 = 0 (pure forward motion) is an ordinary
 *                case; and with -1 in f2 the member of the pencil below that no
 *                finite l reaches is the one whose two free entries are equal,
 *                not the one whose free entries are opposite (every
 *                skew-symmetric F, i.e. every pure translation, when the free
 *                columns are a transposed pair);
 *   cubic        det(l f1 + (1 - l) f2) = det(B + l D), B = f2, D = f1 - f2, = c0
 *                + c1 l + c2 l^2 + c3 l^3 where ck sums the determinants with k
 *                rows taken from D and the others from B;
 *   roots        with cm = max |ck|: |c3| > 1e-12 cm: the monic cubic l^3 + a l^2
 *                + b l + d in closed form, Q = (a^2 - 3 b) / 9, R = (2 a^3 - 9 a b
 *                + 27 d) / 54; for R^2 < Q^3 the three roots -2 sqrt(Q) cos((t +
 *                2 pi k) / 3) - a / 3, t = acos(R / sqrt(Q^3)), k = 0, 1, -1, else
 *                the one root A + Q / A - a / 3 with A = -sign(R) cbrt(|R| +
 *                sqrt(R^2 - Q^3)) (Q / A read as 0 for A = 0); each root then
 *                takes two Newton steps on the monic cubic (a step with a zero
 *                derivative or a non-finite result is skipped).  Otherwise
 *                (leading coefficient <= 1e-12 cm) the quadratic c2 l^2 + c1 l +
 *                c0: q = -(c1 + sign(c1) sqrt(c1^2 - 4 c2 c0)) / 2, roots q / c2
 *                and c0 / q, none for a negative discriminant; with |c2| <=
 *                1e-12 cm too, the root -c0 / c1 if |c1| > 1e-12 cm, else none.
 *                The real roots in ascending l are candidates r = 0, 1, 2: Fn =
 *                l f1 + (1 - l) f2, F = T2^T Fn T1.  A sample without a real
 *                root counts as rejected;
 *   score        the squared Sampson distance in pixels, d2 = (x2^T F x1)^2 /
 *                ((F x1)_1^2 + (F x1)_2^2 + (F^T x2)_1^2 + (F^T x2)_2^2); a
 *                match is an inlier iff d2 is finite and <= thr^2, evaluated
 *                without the division as e^2 <= thr^2 den with thr^2 den finite
 *                and den > 0;
 *   selection    most inliers, ties to the lowest iteration, then to the lowest
 *                root index; rejected samples never win;
 *   refit        the normalised 8-point fit over the winner's inliers: N = sum
 *                of a a^T over the inliers' rows a (as in `system`), accumulated
 *                in a fixed order; its eigenvectors by cyclic Jacobi: a sweep
 *                visits (p, q), p < q, in row-major order, and for Npq != 0
 *                rotates with theta = (Nqq - Npp) / (2 Npq), t = sign(theta) /
 *                (|theta| + sqrt(theta^2 + 1)) (sign(0) = +1), c = 1 / sqrt(t^2 +
 *                1), s = t c; sweeps run while the sum of the squared
 *                off-diagonal entries above the diagonal exceeds 1e-32 times the
 *                sum of the squared diagonal entries, 16 at the most.  Fn = the
 *                eigenvector of the lowest diagonal entry (the first on a tie).
 *                Rank 2: the same Jacobi on Fn^T Fn (3x3), w = the eigenvector of
 *                its lowest eigenvalue, Fn <- Fn - (Fn w) w^T, which zeroes the
 *                smallest singular value.  F = T2^T Fn T1 is kept iff the
 *                winner has at least 8 inliers (fewer leave the fit
 *                under-determined), F is finite and not all zero, and its
 *                inlier count is >= the winner's.
 * Outputs (device): F [npairs][9] row-major, Frobenius norm 1, the entry of
 * largest magnitude positive (the first such entry on a tie); info [npairs][4]
 * = {status, n_inliers, best_iter, refit_kept | root << 8} with root the
 * winning candidate's index; inlier [sum n1] uint8 laid out as
 * posfeat_ransac_homography's.  status 1 (fewer than 7 matches, or every sample
 * rejected): F[p] = 0, info {1, 0, -1, 0}, mask 0.
 * Returns, before any device work: POSFEAT_E_INVALID for a null pointer, a set
 * index out of range, a negative or decreasing set_off, sum n1 past INT32_MAX,
 * iters outside 1..65536, a non-finite or non-positive thr;
 * POSFEAT_E_WORKSPACE for ws_bytes below posfeat_ransac_fundamental_workspace
 * (0 for an invalid table or iteration count).  ws must be 256-B aligned.
 * Three launches whatever npairs; stream-ordered, never synchronises the host;
 * NOT graph-capturable (the pair table is copied from pageable host memory).
 * Deterministic: the same inputs give the same bits, and the result for a
 * pair index does not depend on the other pairs of the list.
 * Limitation: a planar scene or a pure rotation is degenerate for F (the
 * epipolar system of its inliers has a three-dimensional null space, and any
 * member fits them).  The call does not detect this; such pairs are what
 * posfeat_ransac_homography is for.
 * posfeat_ransac_sample_k and posfeat_fundamental_solve7 are host only (no
 * device, no launch).  posfeat_ransac_sample_k writes the first k draws (4 <= k
 * <= 8) of the sampler to out[k]; POSFEAT_E_INVALID for n < k, a null out, k
 * out of range, a negative pair or iter.  posfeat_fundamental_solve7 runs
 * `system` to `roots` on m [7][4] = (x, y, u, v) rows already in normalised
 * coordinates, writes the candidates Fn to F [<= 3][9], each scaled as the
 * outputs above, and returns their number: 0 for a rejected sample,
 * POSFEAT_E_INVALID for a null pointer.  It compiles the text the kernels
 * compile, with the host's acos / cos / cbrt. */
int posfeat_ransac_sample_k(uint64_t seed, int pair, int iter, int n, int k, int32_t *out);
int posfeat_fundamental_solve7(const double *m, double *F);
size_t posfeat_ransac_fundamental_workspace(const int32_t *set_off, int nsets,
                                            const int32_t *pairs, int npairs, int iters);
int posfeat_ransac_fundamental(const float *kp, const int32_t *set_off, int nsets,
                               const int32_t *pairs, int npairs, const int32_t *matches,
                               const int32_t *counts, int iters, double thr, uint64_t seed,
                               double *F, int32_t *info, uint8_t *inlier, void *ws,
                               size_t ws_bytes, void *stream);

/* Feature tracks and one robustly triangulated 3-D point per track from
 * verified matches and known cameras: what the reference's Aachen pipeline
 * asks of `colmap point_triangulator` after geometric_verification
 * (evaluations/aachen/reconstruct_pipeline.py).  All in fp64.
 * set_off (nsets + 1 entries, set_off[0] = 0, not decreasing) is a HOST table;
 * every other pointer is a device pointer.  N = set_off[nsets] pool rows; row r
 * belongs to the set s with set_off[s] <= r < set_off[s + 1]; a set is an image.
 *   kp     [N][2] fp32       pixel (x, y), used as given
 *   cams   [nsets][8] fp64   (fx, fy, cx, cy, k1, 0, 0, 0)
 *   poses  [nsets][12] fp64  [R | t] row-major, world to camera, x_cam = R X + t
 *                            (COLMAP's convention); the centre is C = -R^T t
 *   edges  [nedges][2] int32 global pool rows
 *   camera       once per row.  Undistortion: xd = (x - cx) / fx, yd = (y - cy) /
 *                fy, rd = hypot(xd, yd); for k1 = 0 or rd = 0 the undistorted
 *                point (xu, yu) is (xd, yd); otherwise ru starts at rd and takes
 *                exactly 8 Newton steps ru <- ru - g / g' on g(ru) = ru (1 + k1
 *                ru^2) - rd, g' = 1 + 3 k1 ru^2, a step whose g' is not a
 *                positive finite number skipped, and (xu, yu) = (ru / rd) (xd,
 *                yd).  Projection of X: (xc, yc, z) = R X + t, xn = xc / z, yn =
 *                yc / z, f = 1 + k1 (xn^2 + yn^2), pixel = (fx f xn + cx, fy f yn
 *                + cy).  The reprojection error is the pixel distance to (x, y);
 *                an observation is an inlier of X iff z > 0 and the squared
 *                error is finite and <= thr^2;
 *   tracks       an edge is ignored, before any memory is touched through it,
 *                when an end lies outside [0, N), both ends are in one set, or
 *                both ends are one row.  Duplicate and reversed edges are
 *                harmless.  root(r) = the smallest row of r's connected
 *                component.  A component of 2..max_track rows is a track;
 *                larger ones are dropped (and counted).  Tracks are numbered in
 *                ascending root order, members listed in ascending row order;
 *                nothing depends on the order of `edges`;
 *   DLT          each observation, in a given order, contributes the two
 *                4-vectors a = xu P3 - P1 and b = yu P3 - P2 (Pi the rows of [R |
 *                t]); N4 = sum (a a^T + b b^T), every entry accumulated in that
 *                order (first a's product, then b's); its eigenvectors by the
 *                cyclic Jacobi of posfeat_ransac_fundamental's refit (the same
 *                visiting order, rotation formulas, stopping rule, at most 16
 *                sweeps); v = the eigenvector of the lowest diagonal entry (the
 *                first on a tie).  Rejected when |v4| <= 1e-12 max |vi| or
 *                anything is not finite; else X = (v1, v2, v3) / v4;
 *   hypotheses   a track with members 0..m-1 (ascending rows), root row rho, H
 *                = m (m - 1) / 2.  H <= iters: hypothesis h is the h-th pair (i <
 *                j) in lexicographic order, h = 0..H-1.  Otherwise (then m >= 5)
 *                hypothesis h = 0..iters-1 takes (i, j) = the first two draws of
 *                posfeat_ransac_sample(seed, rho, h, m), as drawn, not sorted.  X
 *                = the DLT of observations i, j in that order.  Rejected when
 *                the DLT rejects, z <= 0 in view i or j, or the angle at X
 *                between X - Ci and X - Cj is below min_angle_deg: with d = (X -
 *                Ci) . (X - Cj) and the two lengths, the test passes iff both
 *                lengths are > 0 and d / (|X - Ci| |X - Cj|) < cos(min_angle_deg)
 *                (two observations in one image never survive);
 *   score        the number of members that are inliers of X;
 *   selection    most inliers, ties to the lowest h; rejected hypotheses never
 *                win;
 *   refit        the DLT over the winner's inliers in member order; kept iff it
 *                is accepted, its own inlier count is >= the winner's, z > 0 in
 *                the winning pair's two views and the winning pair's angle at
 *                the new X passes.  When kept, the flags are the refit's.
 * Outputs (device), Tmax = min(nedges, N / 2), Mmax = min(2 nedges, N):
 *   points [Tmax][3], err [Tmax]: the point and the mean reprojection error in
 *     pixels of its final inliers (their sum in member order over their number;
 *     0 without an inlier);
 *   tinfo [Tmax][4] = {status, n_inliers, best_h, refit_kept}; status 1 (every
 *     hypothesis rejected): point 0, err 0, {1, 0, -1, 0}, flags 0;
 *   track_off [Tmax + 1], track_rows [Mmax], obs_inlier [Mmax] (uint8, parallel
 *     to track_rows): track t has the members track_rows[track_off[t] ..
 *     track_off[t + 1]);
 *   point_of_row [N]: the track id where the row is a final inlier of a status-0
 *     track, else -1;
 *   counts [8] = {T, members, points with status 0, inlier observations, dropped
 *     oversized components, ignored edges, 0, 0}.
 * Entries past T / the member count are not written.  Every output buffer must
 * hold at least one element.
 * Returns, before any device work: POSFEAT_E_INVALID for a null pointer (an
 * input without elements may be null: kp for N = 0, cams and poses for nsets =
 * 0, edges for nedges = 0), a null set_off, nsets < 0, set_off[0] != 0, a
 * decreasing set_off, iters outside 8..1024, max_track outside 2..1024, a
 * non-finite or non-positive thr, min_angle_deg outside [0, 90), a negative
 * nedges, ws not 256-B aligned, points or err not 8-B aligned;
 * POSFEAT_E_WORKSPACE for ws_bytes below
 * posfeat_triangulate_workspace (0 for invalid arguments).  nedges = 0 and N = 0
 * are valid and give counts = 0.  Camera and pose values are data: non-finite
 * entries only make observations fail the inlier test.
 * Nine launches (and one copy of set_off) whatever N, nedges and T;
 * stream-ordered, never synchronises the host; NOT graph-capturable (set_off is
 * copied from pageable host memory).  Deterministic: the same inputs give the
 * same bits, and the result for a track (its point, err, info, members, flags)
 * depends only on its own component's rows, their cameras, seed, iters, thr
 * and min_angle_deg.
 * posfeat_triangulate_dlt is host only (no device, no launch) and compiles the
 * text the kernels compile: obs [n][14] = (xu, yu, the 12 pose entries), n >= 1,
 * to X [3]; returns 0, 1 for a rejected system (X = 0), POSFEAT_E_INVALID for a
 * null pointer or n < 1. */
size_t posfeat_triangulate_workspace(const int32_t *set_off, int nsets, long long nedges,
                                     int max_track);
int posfeat_triangulate(const float *kp, const int32_t *set_off, int nsets, const double *cams,
                        const double *poses, const int32_t *edges, long long nedges, int iters,
                        double thr, double min_angle_deg, int max_track, uint64_t seed,
                        double *points, double *err, int32_t *tinfo, int32_t *track_off,
                        int32_t *track_rows, uint8_t *obs_inlier, int32_t *point_of_row,
                        int32_t *counts, void *ws, size_t ws_bytes, void *stream);
int posfeat_triangulate_dlt(const double *obs, int n, double *X);

/* RANSAC absolute poses for every query of a list from 2D-3D correspondences:
 * what the reference's Aachen pipeline asks of `colmap image_registrator`
 * after the sparse model is built (evaluations/aachen/reconstruct_pipeline.py
 * register_queries).  All in fp64.  q_off (nq + 1 entries, q_off[0] = 0, not
 * decreasing; C = q_off[nq] correspondences) is a HOST table; every other
 * pointer is a device pointer.
 *   kp     [nkp][2] fp32      the queries' keypoint pool, pixel (x, y)
 *   cams   [nq][8] fp64       posfeat_triangulate's camera row, one per query
 *   points [npoints][3] fp64  world points (posfeat_triangulate's `points`, as
 *                             left on the device)
 *   corr   [C][2] int32       (pool row, point index); query q owns rows q_off[q]
 *                             .. q_off[q + 1], numbered 0 .. n - 1 below
 *   rows         a correspondence is invalid when its pool row is outside [0,
 *                nkp), its point index outside [0, npoints), or its pixel,
 *                undistorted point or world point is not finite.  An invalid
 *                correspondence is never an inlier and rejects every sample
 *                that draws it; nothing is read through its indices.  The
 *                undistorted normalised point (xu, yu) is posfeat_triangulate's
 *                `camera` undistortion (exactly 8 Newton steps);
 *   sample       iteration it = 0 .. iters - 1 of query q takes the first three
 *                draws of posfeat_ransac_sample(seed, q, it, n), as drawn: the
 *                correspondences 1, 2, 3 with world points P1, P2, P3 and unit
 *                bearings fi = (xu, yu, 1) / |(xu, yu, 1)|.  A query needs n >=
 *                4.  Rejected when a drawn correspondence is invalid; when |(P2
 *                - P1) x (P3 - P1)| <= 1e-6 |P2 - P1| |P3 - P1| (collinear or
 *                coincident points; a NaN rejects); or when two bearings have a
 *                cosine >= 1 - 1e-12;
 *   quartic      Grunert's: a2 = |P2 - P3|^2, b2 = |P1 - P3|^2, c2 = |P1 - P2|^2,
 *                ca = f2 . f3, cb = f1 . f3, cg = f1 . f2, k = (a2 - c2) / b2, m =
 *                (a2 + c2) / b2; with the depths s2 = u s1, s3 = v s1 the ratio v
 *                solves A4 v^4 + A3 v^3 + A2 v^2 + A1 v + A0 = 0,
 *                  A4 = (k - 1)^2 - 4 (c2 / b2) ca^2
 *                  A3 = 4 [k (1 - k) cb - (1 - m) ca cg + 2 (c2 / b2) ca^2 cb]
 *                  A2 = 2 [k^2 - 1 + 2 k^2 cb^2 + 2 ((b2 - c2) / b2) ca^2
 *                          - 4 m ca cb cg + 2 ((b2 - a2) / b2) cg^2]
 *                  A1 = 4 [-k (1 + k) cb + 2 (a2 / b2) cg^2 cb - (1 - m) ca cg]
 *                  A0 = (1 + k)^2 - 4 (a2 / b2) cg^2;
 *   roots        in closed form, no iteration with a data-dependent trip count.
 *                With cm = max |Ak|: |A4| <= 1e-12 cm: the cubic A3 v^3 + ... + A0
 *                by posfeat_ransac_fundamental's `roots` (closed form, two
 *                Newton steps, its own fall-back to the quadratic and the linear
 *                case).  Otherwise Ferrari: when |A0| > |A4| the coefficients
 *                are reversed first (the quartic in 1 / v; its roots are inverted
 *                at the end and a root 0 is dropped), so that a root far out
 *                does not swamp the others.  The monic quartic y^4 + a y^3 + b
 *                y^2 + c y + d is depressed by y -> y - a / 4 to y^4 + p y^2 + q y
 *                + r, p = b - 3 a^2 / 8, q = c - a b / 2 + a^3 / 8, r = d - a c / 4 +
 *                a^2 b / 16 - 3 a^4 / 256; m = the largest real root of the
 *                resolvent 8 m^3 + 8 p m^2 + (2 p^2 - 8 r) m - q^2 by the same
 *                `roots`.  For a finite m > 0, with s = sqrt(2 m), h = p / 2 + m,
 *                w = q / (2 s), the quartic is (y^2 + s y + h - w)(y^2 - s y + h +
 *                w); a factor y^2 + B y + C with B^2 - 4 C >= 0 gives t = -(B +
 *                sign(B) sqrt(B^2 - 4 C)) / 2 and C / t.  Otherwise the
 *                biquadratic: z^2 + p z + r the same way (second root r / t, 0
 *                for t = 0; none for a negative discriminant), every z >= 0
 *                giving +-sqrt(z).  Every root then takes two Newton steps on
 *                the quartic as given, A4 v^4 + ... + A0 (a step with a zero
 *                derivative or a non-finite result is skipped).  The roots are
 *                sorted ascending and a root within 1e-9 max(1, |v|) of the
 *                last root kept is dropped (roots that close count once);
 *   candidates   a root v is a candidate iff v > 0, u = [(k - 1) v^2 - 2 k cb v
 *                + 1 + k] / (2 (cg - v ca)) is finite and > 0, s1 = sqrt(b2 / (1
 *                + v^2 - 2 v cb)) is finite and > 0, and its pose is finite.
 *                With the camera points Qi = si fi, the triad of three points
 *                (A, B, C) is e1 = (B - A) / |B - A|, e3 = e1 x (C - A)
 *                normalised, e2 = e3 x e1, T = [e1 e2 e3] (columns): R = T(Q1,
 *                Q2, Q3) T(P1, P2, P3)^T, t = Q1 - R P1.  At most four
 *                candidates, numbered r = 0 .. 3 in ascending v;
 *   score        the number of correspondences that are inliers of [R | t]:
 *                with (xc, yc, z) = R X + t, z > 0 and the squared pixel
 *                reprojection error (posfeat_triangulate's `camera`
 *                projection, distortion included) finite and <= thr^2.  It is
 *                evaluated without the division: with g = z^2 + k1 (xc^2 +
 *                yc^2), xd = (x - cx) / fx, yd = (y - cy) / fy, the error times
 *                z^3 is (fx (xc g - xd z^3), fy (yc g - yd z^3)), compared with
 *                thr^2 z^6 (which must be finite);
 *   selection    most inliers, ties to the lowest iteration, then to the lowest
 *                candidate number; rejected samples never win;
 *   refit        Gauss-Newton on the pixel reprojection error over the winner's
 *                inliers (the set stays fixed), attempted iff there are at
 *                least 4.  The unknowns delta = (omega, tau) perturb a camera
 *                point as Xc + omega x Xc + tau.  Per inlier the residual r =
 *                projection - (x, y) and its 2 x 6 Jacobian J = (d pixel / d
 *                Xc) [-[Xc]x | I]; N = sum J^T J (upper triangle), g = sum J^T
 *                r and the cost sum |r|^2 are accumulated in a fixed order.  N
 *                delta = -g by Gaussian elimination with partial pivoting (the
 *                first largest entry of the column); a pivot below 1e-12 times
 *                the largest entry of its column of N, or not positive, or a
 *                non-finite delta, stops the refit.  The step R <- exp(omega) R,
 *                t <- exp(omega) t + tau (Rodrigues: exp = I + (sin th / th) K +
 *                (2 sin^2(th / 2) / th^2) K^2, K = [omega]x, th = |omega|; I + K
 *                + K^2 / 2 for th = 0) is taken iff at the new pose every
 *                inlier has z > 0 and a finite residual and the cost is lower;
 *                a refused step stops the refit.  At most 10 steps; after a
 *                step with max |delta_i| <= 1e-12 it stops too.  The refit's
 *                pose is kept iff it is finite and its own inlier count (over
 *                all correspondences) is >= the winner's; the mask is then the
 *                refit's.
 * Outputs (device): poses [nq][12] = [R | t] row-major, world to camera; info
 * [nq][4] = {status, n_inliers, best_iter, refit_kept | root << 8} with root the
 * winning candidate's number; inlier [C] uint8 parallel to corr.  status 1
 * (fewer than 4 correspondences, or every sample rejected): pose 0, info {1, 0,
 * -1, 0}, mask 0.
 * Returns, before any device work: POSFEAT_E_INVALID for a null pointer, nq < 0,
 * q_off[0] != 0, a decreasing q_off, nkp or npoints < 0, iters outside 1..65536,
 * a non-finite or non-positive thr, ws not 256-B aligned, poses, points or cams
 * not 8-B aligned, info or corr not 4-B aligned; POSFEAT_E_WORKSPACE for
 * ws_bytes below posfeat_ransac_pose_workspace (0 for an invalid table or
 * iteration count).  nq = 0 is valid and does nothing.
 * Three launches (and one copy of q_off) whatever nq; stream-ordered, never
 * synchronises the host; NOT graph-capturable (q_off is copied from pageable
 * host memory).  Deterministic: the same inputs give the same bits, and the
 * result for a query index depends only on that index, its own correspondences
 * and camera, seed, iters and thr.
 * posfeat_pose_solve3 is host only (no device, no launch) and compiles the text
 * the kernels compile, with the host's acos / cos / cbrt: it runs `sample`'s
 * rejections to `candidates` on m [3][5] = (xu, yu, X, Y, Z) rows, writes the
 * candidate poses to poses [<= 4][12] and returns their number: 0 for a rejected
 * sample, POSFEAT_E_INVALID for a null pointer. */
size_t posfeat_ransac_pose_workspace(const int32_t *q_off, int nq, int iters);
int posfeat_ransac_pose(const float *kp, long long nkp, const double *cams, const double *points,
                        long long npoints, const int32_t *corr, const int32_t *q_off, int nq,
                        int iters, double thr, uint64_t seed, double *poses, int32_t *info,
                        uint8_t *inlier, void *ws, size_t ws_bytes, void *stream);
int posfeat_pose_solve3(const double *m, double *poses);

/* Points-only bundle adjustment of the tracks of posfeat_triangulate: what
 * `colmap point_triangulator` goes on to do with fixed database poses and
 * --Mapper.ba_refine_focal_length 0 --Mapper.ba_refine_principal_point 0
 * --Mapper.ba_refine_extra_params 0 (evaluations/aachen/reconstruct_pipeline.py):
 * the bundle adjustment moves only the points, observations are filtered by
 * reprojection error and points by triangulation angle, again while the model
 * changes.  One independent problem per track.  All in fp64.
 * set_off is a HOST table; every other pointer is a device pointer.
 *   kp, set_off, nsets, cams, poses   as posfeat_triangulate takes them, N =
 *                set_off[nsets] pool rows
 *   points_in [tmax][3], tinfo_in [tmax][4], track_off [tmax + 1], track_rows
 *   [mmax], inlier_in [mmax], counts_in [8]   what a posfeat_triangulate call
 *                left (its points, tinfo, track_off, track_rows, obs_inlier,
 *                counts); T = counts_in[0] clamped to [0, tmax] is read on the
 *                device.  None of them is written.  tmax, mmax are the
 *                capacities of the buffers (posfeat_triangulate's Tmax, Mmax).
 *                Track t has the m = track_off[t + 1] - track_off[t] members
 *                track_rows[track_off[t] ..], numbered 0 .. m - 1 below; a
 *                flag is set when its byte is not 0.  A member whose row is
 *                outside [0, N) is never an inlier, is in no set, and nothing is
 *                read through it.  A track whose range is not inside [0, mmax]
 *                or has more than 1024 members (not posfeat_triangulate's) is
 *                given status 1 and its flags are not written;
 *   residual     of member row r in set s at the point X: posfeat_triangulate's
 *                `camera` projection of X (distortion included) minus the
 *                stored pixel, r = pixel(R_s X + t_s) - (x, y), and its 2 x 3
 *                Jacobian J = (d pixel / d Xc) R_s with d pixel / d Xc the
 *                expression of posfeat_ransac_pose's refit: with xn = xc / z, yn
 *                = yc / z, f = 1 + k1 (xn^2 + yn^2), axx = fx (f + 2 k1 xn^2), axy
 *                = fx 2 k1 xn yn, ayx = fy 2 k1 xn yn, ayy = fy (f + 2 k1 yn^2):
 *                d px / d Xc = (axx, axy, -(axx xn + axy yn)) / z, d py / d Xc =
 *                (ayx, ayy, -(ayx xn + ayy yn)) / z;
 *   sums         over a set S of members at X: N3 = sum J^T J (six entries,
 *                upper triangle), g = sum J^T r, cost = sum |r|^2; per member
 *                each entry takes first the x row's product, then the y row's.
 *                The order depends only on m: for m <= 16 the members of S in
 *                ascending member order into one sum; for m > 16 member k of S
 *                adds to partial sum k mod 64 in ascending k, and the 64
 *                partial sums v[0..63] are combined by v[l] <- v[l] + v[l xor
 *                o] for o = 32, 16, 8, 4, 2, 1 (every v[l] then holds the same
 *                bits).  S is usable at X iff every member of S has z > 0 and a
 *                finite |r|^2 there;
 *   round        Levenberg-Marquardt on X over a fixed S of at least 2 members
 *                (a smaller S leaves X alone).  Nothing happens when S is not
 *                usable at the start.  lambda = 1e-4.  While fewer than `steps`
 *                trial points have been evaluated and lambda <= 1e8: solve (N3
 *                + lambda diag N3) delta = -g by Gaussian elimination with the
 *                pivot rule of posfeat_ransac_pose's refit (partial pivoting,
 *                the first largest entry of the column; a pivot below 1e-12
 *                times the largest entry of its column of the damped matrix, or
 *                not positive, or a non-finite delta: unsolvable, no trial
 *                point is evaluated).  The step to X + delta is taken iff S is
 *                usable there and the cost is strictly lower; then lambda <-
 *                lambda / 10, and the round ends if max |delta_i| <= 1e-10
 *                max(1, max |X_i|) at the new X.  A refused or unsolvable step
 *                gives lambda <- 10 lambda.  The cost over S never rises;
 *   rounds       a track whose input status is not 0 is carried through as
 *                status 1.  X starts as the input point, S_1 as the input flags
 *                (valid rows only).  Round k = 1 .. rounds: the LM round on S_k;
 *                then every member of the track is tested at X by
 *                posfeat_triangulate's inlier rule (thr), which gives F.  |F| <
 *                2: status 2, stop.  F = S_k: converged, stop.  Otherwise S_k+1
 *                = F.  The output flags are the last F; err is the mean pixel
 *                error over F at the final X (the sum in member order over
 *                |F|);
 *   angle        COLMAP's filter, not the winning-pair rule: a point that is
 *                not status 2 survives iff some pair i < j of the last F passes
 *                posfeat_triangulate's angle test at X (both |X - C| > 0 and
 *                the cosine < cos(min_angle_deg)); otherwise status 3.  Two rows
 *                of one image never qualify (their centres coincide).
 * Outputs (device, buffers of their own: no output may overlap an input):
 *   points [tmax][3], err [tmax];
 *   tinfo [tmax][4] = {status, n_inliers, best_h and refit_kept of tinfo_in};
 *   obs_inlier [mmax] (parallel to track_rows), point_of_row [N] (the track id
 *     where the row is a final inlier of a status-0 track, else -1);
 *   rinfo [tmax][4] = {rounds used, taken steps, converged, flags changed (the
 *     last F differs from the input flags)}, {0, 0, 0, 0} for a carried track;
 *   counts [8] = {T, status-0 points, their inlier observations, status-2
 *     points, status-3 points, carried status-1 points, tracks whose flags
 *     changed, 0}.
 * A track of status != 0 has point 0, err 0, n_inliers 0 and flags 0, as
 * posfeat_triangulate writes a status-1 track.  Entries past T / the last
 * track's members are not written.  track_off and track_rows are shared with
 * the input, so the result reads like a posfeat_triangulate result.
 * Returns, before any device work: POSFEAT_E_INVALID for a null pointer (kp for
 * N = 0 and cams, poses for nsets = 0 may be null), a bad set table, tmax or
 * mmax negative, tmax + 1 or mmax above INT32_MAX, a non-finite or non-positive thr,
 * min_angle_deg outside [0, 90), rounds outside 1..8, steps outside 1..32, ws
 * not 256-B aligned, points_in, points, err, cams or poses not 8-B aligned, an
 * int32 buffer or kp not 4-B aligned; POSFEAT_E_WORKSPACE for ws_bytes below
 * posfeat_refine_points_workspace (0 for invalid arguments).
 * Three launches (and one copy of set_off) whatever T; stream-ordered, never
 * synchronises the host; NOT graph-capturable (set_off is copied from pageable
 * host memory).  No floating-point atomics.  Deterministic: the same inputs give
 * the same bits, and the result for a track depends only on its own members,
 * their cameras, its input point and flags, thr, min_angle_deg, rounds, steps.
 * posfeat_refine_point is host only (no device, no launch) and compiles the
 * text the kernels compile: one `round` over all n rows of obs [n][22] = (x, y,
 * the 8 camera entries, the 12 pose entries) in the order a track of n members
 * has, from X0 [3]; writes X [3] and the cost there (NaN when the rows are not
 * usable at X0) and returns the number of taken steps; POSFEAT_E_INVALID for a
 * null pointer, n < 2 or steps outside 1..32. */
size_t posfeat_refine_points_workspace(const int32_t *set_off, int nsets, long long tmax,
                                       long long mmax);
int posfeat_refine_points(const float *kp, const int32_t *set_off, int nsets, const double *cams,
                          const double *poses, const double *points_in, const int32_t *tinfo_in,
                          const int32_t *track_off, const int32_t *track_rows,
                          const uint8_t *inlier_in, const int32_t *counts_in, long long tmax,
                          long long mmax, double thr, double min_angle_deg, int rounds, int steps,
                          double *points, double *err, int32_t *tinfo, uint8_t *obs_inlier,
                          int32_t *point_of_row, int32_t *rinfo, int32_t *counts, void *ws,
                          size_t ws_bytes, void *stream);
int posfeat_refine_point(const double *obs, int n, const double *X0, int steps, double *X,
                         double *cost);

/* Split tracks: sequential RANSAC over the members a track's RANSAC left out.
 * posfeat_triangulate makes one point per connected component of the match
 * graph and drops every member that is not an inlier of it; in `colmap
 * point_triangulator`, the step that call stands in for, an observation that
 * did not join a point stays free and is triangulated again with its own
 * correspondences.  One wrong verified match that ties two real tracks together
 * costs the smaller one there; this call gets it back.  Opt-in: it takes a
 * posfeat_triangulate result and returns a result of the same shape in which a
 * track may have become several.  All in fp64.
 * set_off is a HOST table; every other pointer is a device pointer.
 *   kp, set_off, nsets, cams, poses   as posfeat_triangulate takes them, N =
 *                set_off[nsets] pool rows
 *   points_in [tmax][3], err_in [tmax], tinfo_in [tmax][4], track_off_in [tmax
 *   + 1], track_rows_in [mmax], inlier_in [mmax], counts_in [8]   what a
 *                posfeat_triangulate call left (its points, err, tinfo,
 *                track_off, track_rows, obs_inlier, counts); T = counts_in[0]
 *                clamped to [0, tmax] is read on the device.  None of them is
 *                written.  tmax, mmax are the capacities of the buffers
 *                (posfeat_triangulate's Tmax, Mmax).  A flag is set when its
 *                byte is not 0;
 *   iters, thr, min_angle_deg, seed   posfeat_triangulate's, with its ranges;
 *   rounds       1..4: the generations a track runs at the most;
 *   tmax_out     >= tmax: the track capacity of the output;
 *   parents      an input track ("parent") t has the m members track_rows_in[
 *                track_off_in[t] ..], numbered 0 .. m - 1 in that order, which
 *                is ascending row order in a posfeat_triangulate result.  Its
 *                left-over list L_1 is its unflagged members in member order.
 *                A parent is carried through unchanged when its status is not
 *                0, when |L_1| < 2, or when its member range is not inside [0,
 *                mmax] or has more than 1024 members (posfeat_refine_points'
 *                rule: nothing is read or written through such a range, so the
 *                range of the output track_rows and obs_inlier is not written
 *                either);
 *   generations  generation g = 1 .. rounds takes L_g while |L_g| >= 2 and runs
 *                exactly posfeat_triangulate's `hypotheses`, `score`,
 *                `selection` and `refit` on L_g as if L_g were a track: the
 *                members of L_g in order, rho = L_g[0], the same seed and the
 *                same rule for iters (the same device functions).  A member
 *                whose row is outside [0, N) is never an inlier and nothing is
 *                read through it: a hypothesis whose pair holds one is
 *                rejected.  If every hypothesis is rejected, or fewer than 2
 *                members are inliers of the final point, the parent stops.
 *                Otherwise child g exists: that point, err as
 *                posfeat_triangulate defines it, tinfo {0, n_inliers, best_h,
 *                refit_kept}, and its members are those final inliers.  L_g+1 =
 *                L_g without them, in order;
 *   numbering    parent t with c_t children becomes 1 + c_t output tracks, in
 *                this order: the parent, child 1 .. c_t; the output tracks are
 *                numbered in parent order by a scan on the device.  Under the
 *                capacity: walking the tracks in output order, a child is
 *                created iff its number plus the number of parents after its
 *                own stays below tmax_out, so every parent has a place
 *                whatever the children before it; the children that are not
 *                created are then the last ones in output order.  The rows of
 *                a child that is not created stay with the parent;
 *   partition    the members of a parent and of its created children together
 *                occupy the parent's range of track_rows_in, parent first; each
 *                output track lists its members in member order.  A child's
 *                members are its inliers, all flagged 1.  The parent keeps
 *                every member no created child claimed (its own inliers and
 *                the final left-overs) with their input flag bytes, and its
 *                point, err and tinfo bit for bit.  So every member row of
 *                the input is a member of exactly one output track.
 * Outputs (device, buffers of their own: no output may overlap an input):
 *   points [tmax_out][3], err [tmax_out], tinfo [tmax_out][4];
 *   track_off [tmax_out + 1], track_rows [mmax], obs_inlier [mmax];
 *   point_of_row [N]: the output id of the status-0 track in which the row is
 *     a flagged member, else -1 (the input's point_of_row under the new
 *     numbering, plus the child's id for each child inlier);
 *   parent_of [tmax_out], generation [tmax_out]: the input track id, and 0 for
 *     the parent itself, g for child g;
 *   counts [8] = {T', members (counts_in[1]), tracks with status 0, the sum of
 *     their n_inliers, children that did not fit in tmax_out, 0, children
 *     created, parents with at least one created child}; the first four as
 *     posfeat_triangulate lays them out.  Disjoint tracks of at least two
 *     members give T' <= mmax / 2.
 * Entries past T' / the member count are not written.
 * Out of scope: a component larger than max_track is still dropped by
 * posfeat_triangulate, and a status-1 parent is not tried again.
 * Returns, before any device work: POSFEAT_E_INVALID for a null pointer (kp for
 * N = 0 and cams, poses for nsets = 0 may be null), a bad set table, tmax or
 * mmax negative, tmax + 1 or mmax above INT32_MAX, tmax_out below tmax or
 * tmax_out + 1 above INT32_MAX, iters outside 8..1024, a non-finite or
 * non-positive thr, min_angle_deg outside [0, 90), rounds outside 1..4, an
 * output pointer equal to the input of the same name, ws not 256-B aligned, an
 * fp64 buffer not 8-B aligned, an int32 buffer or kp not 4-B aligned;
 * POSFEAT_E_WORKSPACE for ws_bytes below posfeat_split_tracks_workspace (0 for
 * invalid arguments).
 * Seven launches (and one copy of set_off) whatever T; stream-ordered, never
 * synchronises the host; NOT graph-capturable (set_off is copied from pageable
 * host memory).  No floating-point atomics.  Deterministic: the same inputs give
 * the same bits, and what a parent becomes (its children, their points and
 * members) depends only on its own members, their cameras, its input flags,
 * iters, thr, min_angle_deg, seed and rounds (and, for the children that fit,
 * on tmax_out). */
size_t posfeat_split_tracks_workspace(const int32_t *set_off, int nsets, long long tmax,
                                      long long mmax, long long tmax_out);
int posfeat_split_tracks(const float *kp, const int32_t *set_off, int nsets, const double *cams,
                         const double *poses, const double *points_in, const double *err_in,
                         const int32_t *tinfo_in, const int32_t *track_off_in,
                         const int32_t *track_rows_in, const uint8_t *inlier_in,
                         const int32_t *counts_in, long long tmax, long long mmax, int iters,
                         double thr, double min_angle_deg, uint64_t seed, int rounds,
                         long long tmax_out, double *points, double *err, int32_t *tinfo,
                         int32_t *track_off, int32_t *track_rows, uint8_t *obs_inlier,
                         int32_t *point_of_row, int32_t *parent_of, int32_t *generation,
                         int32_t *counts, void *ws, size_t ws_bytes, void *stream);

/* Five-point RANSAC essential matrices and relative poses for every pair of a
 * list whose cameras are calibrated: the two-view problem between
 * posfeat_ransac_fundamental (no calibration) and posfeat_triangulate (known
 * poses), and what a relative-pose AUC is computed from.  kp, set_off, pairs,
 * matches, counts, iters, seed, ws and stream mean what they mean for
 * posfeat_ransac_fundamental; cams [nsets][8] fp64 is posfeat_triangulate's
 * camera row (fx, fy, cx, cy, k1, 0, 0, 0), one per set, on the device.  Per
 * pair p = (s1, s2) with n = counts[p] matches, all in fp64, contraction off:
 *   coordinates  every match whose indices are inside their sets is
 *                undistorted on both sides as posfeat_triangulate undistorts
 *                (8 Newton steps on the SIMPLE_RADIAL model) into normalised
 *                camera coordinates x1 = (x, y, 1), x2 = (u, v, 1).  A match
 *                outside its sets, or with a non-finite undistorted point, is
 *                a NaN row: it rejects any sample that draws it and is never
 *                an inlier.  No further normalisation: calibrated coordinates
 *                are of order one;
 *   threshold    COLMAP's rule for calibrated pairs: thr_n = (thr / f1 + thr /
 *                f2) / 2 with fi = (fx_i + fy_i) / 2, thr in pixels;
 *   sampler      iteration `it` draws the five distinct match indices
 *                posfeat_ransac_sample_k(seed, p, it, n, 5, out) gives;
 *   system       row i of the 5x9 system A e = 0 is (u x, u y, u, v x, v y, v,
 *                x, y, 1) of sample match i, e = E row-major (x2^T E x1 = 0);
 *   null space   posfeat_ransac_fundamental's elimination with full pivoting
 *                (the same pivot, tie and 1e-12 rejection rule) over s = 0..4;
 *                the four columns left at positions 5..8 are free: e_j (j =
 *                0..3) has 1 at position 5 + j and 0 at the other three, the
 *                rest by back substitution, then the column swaps undone.  The
 *                basis is E_i = sum_j M[i][j] e_j with the fixed orthogonal M =
 *                I - w w^T / 27, w = (-2, -4, -5, 3), whose last row is (2, 4,
 *                5, 6) / 9 (the sum over j in ascending order, each M[i][j] the
 *                quotient of an integer by 27);
 *   constraints  E = x E_0 + y E_1 + z E_2 + E_3.  Linear polynomials are held
 *                over (x, y, z, 1), quadratic ones over (x^2, xy, xz, x, y^2,
 *                yz, y, z^2, z, 1), cubic ones over the twenty monomials (x^3,
 *                y^3, x^2 y, x y^2, x^2 z, x^2, y^2 z, y^2, xyz, xy, x z^2, xz,
 *                x, y z^2, yz, y, z^3, z^2, z, 1).  A product of two linear
 *                polynomials sums a[i] b[j] over i then j; a cubic accumulates
 *                s (q[k] l[j]) over k then j.  Row 0 of the 10x20 matrix is det
 *                E expanded along its first row (minors (E11 E22 - E12 E21),
 *                (E10 E22 - E12 E20), (E10 E21 - E11 E20), signs + - +); row 1 +
 *                3 i + j is the entry (i, j) of 2 E E^T E - tr(E E^T) E, with (E
 *                E^T)_ik the sum of three products in column order, the three
 *                terms 2 (E E^T)_ik E_kj in k order and then -tr E_ij;
 *   elimination  Nister's route: Gauss-Jordan on the first ten columns with
 *                partial pivoting (the first largest |entry| of column s in
 *                rows >= s; row s divided by it; column s cleared in every
 *                other row).  The sample is rejected when a pivot is below
 *                1e-12 times the largest |entry| of the matrix as formed or is
 *                not a positive number.  With e..j rows 4..9 of the result, the
 *                rows e - z f, g - z h, i - z j form the 3x3 matrix B(z) whose
 *                columns multiply (x, y, 1), of degrees (3, 3, 4) in z; its
 *                determinant, expanded along the first row with polynomial
 *                products summed over i then j, is the degree-10 polynomial c;
 *   roots        no root when a coefficient is not finite or |c10| <= 1e-12
 *                max |ck|.  On the monic a = c / c10, Aberth-Ehrlich in complex
 *                arithmetic (products and quotients by the textbook formulas):
 *                the ten estimates start at r0 (cos t_k, sin t_k), t_k = 2 pi k
 *                / 10 + 0.7, r0 = max_k |a[10-k]|^(1/k) (1 when that is 0); a
 *                sweep visits i = 0..9 in order, each with the estimates as
 *                they stand: p and p' at z_i by Horner, nothing for p = 0, else
 *                w = p / p', s = sum_{j != i} 1 / (z_i - z_j), z_i -= w / (1 - w
 *                s) when that is finite.  40 sweeps, always all of them: a
 *                fixed operation count, the same text on host and device, no
 *                library eigen-solver.  z_i is real iff |Im z_i| <= 1e-8 max(1,
 *                |z_i|); its real part then takes two Newton steps on the real
 *                monic polynomial (a step with a zero derivative or a
 *                non-finite result is skipped).  Per real root in ascending z:
 *                B(z) by Horner, the cross products of its rows (0, 1), (0, 2),
 *                (1, 2); the first with the largest |third component| gives x =
 *                c0 / c2, y = c1 / c2.  (x, y, z) then takes three Gauss-Newton
 *                steps on the ten cubics themselves (the 10x20 matrix as it
 *                was before the elimination): mon_k = (x^a y^b) z^c, r = A mon,
 *                J = A dmon/d(x, y, z), N = J^T J, g = J^T r, delta = adj(N) g /
 *                det N by cofactors, (x, y, z) -= delta; a step with a zero
 *                determinant or a non-finite delta is skipped.  This removes
 *                the rounding the elimination and the polynomial's coefficients
 *                leave on an ill-conditioned sample.  E = ((x E_0 + y E_1) + z
 *                E_2) + E_3,
 *                scaled to Frobenius norm 1 with the first largest entry
 *                positive.  A root whose E is not finite or zero is dropped.
 *                The survivors in that order are candidates 0..9; a sample
 *                without one counts as rejected;
 *   score        a match is an inlier iff its squared Sampson distance under E
 *                in normalised coordinates is finite and <= thr_n^2,
 *                evaluated as posfeat_ransac_fundamental evaluates it;
 *   selection    most inliers, ties to the lowest iteration, then to the lowest
 *                candidate index;
 *   refit        the linear fit over the winner's inliers exactly as
 *                posfeat_ransac_fundamental's refit (normal matrix of the rows
 *                of `system` in a fixed order, 9x9 Jacobi, rank 2), in the
 *                normalised camera coordinates themselves; then `project`, then
 *                the output scaling.  Kept iff the winner has at least 8
 *                inliers, the result is finite and not zero, and its inlier
 *                count is >= the winner's;
 *   project      the same Jacobi on E^T E (3x3); v1, v2 the eigenvectors of
 *                the largest and second largest diagonal entry (the first of
 *                equal ones first), v3 = v1 x v2; u_i = E v_i / |E v_i| for i =
 *                1, 2, u3 = u1 x u2; E <- u1 v1^T + u2 v2^T.  The two largest
 *                singular values of an essential matrix are equal, so which
 *                eigenvector comes first is decided by rounding: when the
 *                first largest-magnitude entry of u3 is negative, (u1, u2) and
 *                (v1, v2) are swapped and u3, v3 negated.  U = (u1 u2 u3) and
 *                V = (v1 v2 v3) have determinant +1;
 *   pose         U and V of `project` run on the output E.  The four
 *                decompositions in the order (U W V^T, +u3), (U W V^T, -u3), (U
 *                W^T V^T, +u3), (U W^T V^T, -u3), W = [0 -1 0; 1 0 0; 0 0 1].
 *                For each, every inlier match is triangulated between [I | 0]
 *                and [R | t]: with a = R x1, the two rows d1 (a0 - u a2) = u t2
 *                - t0 and d1 (a1 - v a2) = v t2 - t1 give the least-squares
 *                depth d1 = (p . q) / (p . p) in view 1, and d2 = r3 . (d1 x1) +
 *                t2 in view 2 (posfeat_triangulate's depth).  A match is in
 *                front when both are finite and positive; the decomposition
 *                with the most such inliers wins, ties to the lowest index.
 * Outputs (device): E [npairs][9] row-major, scaled as above; pose [npairs][12]
 * the row-major [R | t] with x2 ~ R x1 + t and |t| = 1; info [npairs][4] =
 * {status, n_inliers, best_iter, refit_kept | root << 8}; cheir [npairs][2] =
 * {decomposition index, n_front}; inlier as posfeat_ransac_fundamental lays it
 * out.  status 1 (fewer than 5 matches, or every sample rejected): E and pose
 * 0, info {1, 0, -1, 0}, cheir {-1, 0}, mask 0.
 * Returns, before any device work, what posfeat_ransac_fundamental returns for
 * the same mistakes (a null cams is one); E, pose and cams must be 8-B aligned.
 * posfeat_ransac_essential_workspace is 0 for an invalid table or iteration
 * count; the workspace holds 10 candidate records of 80 B per iteration and
 * pair, about 0.8 MB per pair at 1024 iterations.
 * Four launches (and one copy of the pair table) whatever npairs;
 * stream-ordered, never synchronises the host; NOT graph-capturable.  No
 * atomics.  Deterministic: the same inputs give the same bits, and the result
 * for a pair index does not depend on the other pairs of the list.
 * Limitations: the gauge (coefficient 1 on E_3) cannot reach a solution whose
 * free entries f satisfy 2 f5 + 4 f6 + 5 f7 + 6 f8 = 0; M is there so that no
 * zero pattern and no symmetric or skew-symmetric pair of entries (every pure
 * translation) produces this, which leaves a measure-zero set.  Under pure
 * rotation every t fits: the inlier count is still well defined, the pose's t
 * is not, and n_front is not meaningful.
 * posfeat_essential_solve5 and posfeat_essential_decompose are host only (no
 * device, no launch) and compile the text the kernels compile, with the host's
 * pow.  posfeat_essential_solve5 runs `system` to `roots` on m [5][4] = (x, y,
 * u, v) rows in normalised camera coordinates, writes the candidates to E [<=
 * 10][9] and returns their number: 0 for a rejected sample or a non-finite
 * row, POSFEAT_E_INVALID for a null pointer.  posfeat_essential_decompose runs
 * `pose` on E [9] over all n rows of m [n][4], writes pose [12] and front [2] =
 * {decomposition index, n_front}; POSFEAT_E_INVALID for a null pointer (m may
 * be null for n = 0), n < 0, or an E whose decompositions are not finite. */
int posfeat_essential_solve5(const double *m, double *E);
int posfeat_essential_decompose(const double *E, const double *m, int n, double *pose,
                                int32_t *front);
size_t posfeat_ransac_essential_workspace(const int32_t *set_off, int nsets,
                                          const int32_t *pairs, int npairs, int iters);
int posfeat_ransac_essential(const float *kp, const double *cams, const int32_t *set_off,
                             int nsets, const int32_t *pairs, int npairs,
                             const int32_t *matches, const int32_t *counts, int iters,
                             double thr, uint64_t seed, double *E, double *pose, int32_t *info,
                             int32_t *cheir, uint8_t *inlier, void *ws, size_t ws_bytes,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* POSFEAT_HIP_H */
