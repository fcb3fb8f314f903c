/*
 * genpose_hip.h -- C ABI of libgenpose_hip.so, the MI355X (gfx950) implementation of the
 * GenPose++ pose-candidate path.
 *
 * Conventions (replacing the reference's pybind module `pointnet2_cuda`,
 * networks/pts_encoder/pointnet2_utils/pointnet2/src/pointnet2_api.cpp:10-24):
 *   - every pointer argument is caller-owned DEVICE memory unless marked "host";
 *     the library never allocates inside a call (workspaces are sized by *_workspace_size);
 *   - every call is enqueued on `stream` and returns immediately (no device sync);
 *   - every call returns 0 (GP_OK) or a negative status; gp_last_error() (thread-local)
 *     describes the failure. Nothing calls exit() (the reference launchers do, e.g.
 *     src/ball_query_gpu.cu:61-65);
 *   - calls are stateless and re-entrant across distinct streams.
 * Layouts are row-major; "packed" weights are produced by genpose2_amd/pack.py.
 */
#ifndef GENPOSE_HIP_H
#define GENPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { GP_OK = 0, GP_ERR_INVALID = -1, GP_ERR_LAUNCH = -2, GP_ERR_UNSUPPORTED = -3 };

/* Thread-local description of the last failure (empty string if none). */
const char *gp_last_error(void);
/* ABI version of this header. */
int gp_abi_version(void);
#define GP_ABI_VERSION 7

/* ===================================================================== operator level
 * Drop-in forward ops of `pointnet2_cuda` (same argument meaning and layouts). */

/* furthest_point_sampling_wrapper(b, n, m, points, temp, idx)  src/sampling.cpp / sampling_gpu.cu:94-253
 * xyz (b,n,3) fp32, idx (b,m) int32. `temp` (b,n) is accepted for signature parity and may be
 * NULL: the kernel keeps the running min-distance on chip. Tie rule identical to the reference
 * (strict > within a thread, lower reduction slot on ties, block size min(2^floor(log2 n),1024)). */
int gp_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp, int *idx,
                               hipStream_t stream);

/* gather_points_wrapper(b, c, n, npoints, points, idx, out)  src/sampling_gpu.cu:8-44
 * points (b,c,n), idx (b,npoints) int32 -> out (b,c,npoints). */
int gp_gather_points(int b, int c, int n, int npoints, const float *points, const int *idx,
                     float *out, hipStream_t stream);

/* ball_query_wrapper(b, n, m, radius, nsample, new_xyz, xyz, idx)  src/ball_query_gpu.cu:9-66
 * new_xyz (b,m,3), xyz (b,n,3) -> idx (b,m,nsample) int32: first nsample points with
 * d^2 < radius^2 in index order, padded with the first hit, 0 when there is no hit. */
int gp_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                  const float *xyz, int *idx, hipStream_t stream);

/* group_points_wrapper(b, c, n, npoints, nsample, points, idx, out)  src/group_points_gpu.cu:47-85
 * points (b,c,n), idx (b,npoints,nsample) -> out (b,c,npoints,nsample). */
int gp_group_points(int b, int c, int n, int npoints, int nsample, const float *points,
                    const int *idx, float *out, hipStream_t stream);

/* ===================================================================== fused encoder
 * Pointnet2ClsMSG(0) with the Light config (networks/pts_encoder/pointnet2.py:211-252).
 * `wbuf` holds all packed, BN-folded layers; `layer_off` (HOST, int64 [5][2][3][4]) gives, for
 * layer i of branch b of level l, {float offset of the fp32 A fragments, float offset of the bias
 * (padded to 32), float offset of the split-f16 hi/lo planes or -1, their power-of-two exponent}
 * (-1 = absent). Levels 2-3 run as split-f16 MFMA (per-column activation scaling) when all four of
 * their layer-1/2 plane offsets are given, exact fp32 MFMA otherwise. ABI 5: the [..][4] table;
 * a [5][2][3][2] table of ABI <= 3 is no longer accepted. The exponents are weight-derived state: a
 * host that receives the weights from another rank must receive this table too. */
size_t gp_encoder_workspace_size(int b, int n);
/* HOST out: byte offsets in the workspace of, per level l<4: fps idx (b,M_l) int32,
 * new_xyz (b,M_l,3) fp32, ball idx branch0/1 (b,M_l,ns) int32; and per level l<5 the level
 * features (b,M_l,C_l) point-major fp32.  offsets[l*5 + {0..4}] = {fps, new_xyz, ball0, ball1, feat}. */
int gp_encoder_workspace_layout(int b, int n, int64_t *offsets);
/* pts (b,n,3) un-centred points -> feat (b,1024). */
int gp_encoder_forward(const float *wbuf, const int64_t *layer_off, const float *pts, int b, int n,
                       void *workspace, size_t workspace_bytes, float *feat, hipStream_t stream);
/* Two models over the same points (the ScoreNet and EnergyNet encoders of one batch) share the geometry
 * -- FPS indices, centroids and ball lists depend only on the points. gp_encoder_geometry runs the FPS
 * chain of all four levels and the ball lists of every level into `workspace`; gp_encoder_forward_geom
 * is gp_encoder_forward with that geometry read from `geometry` (a workspace of the same (b, n) layout
 * that gp_encoder_geometry filled, possibly `workspace` itself) and only the per-level MLPs run, their
 * scratch in `workspace`. Same results as gp_encoder_forward, bit for bit. */
int gp_encoder_geometry(const float *pts, int b, int n, void *workspace, size_t workspace_bytes,
                        hipStream_t stream);
int gp_encoder_forward_geom(const float *wbuf, const int64_t *layer_off, const float *pts, int b, int n,
                            const void *geometry, void *workspace, size_t workspace_bytes, float *feat,
                            hipStream_t stream);
/* The same two calls over a range of levels, so that level 0's MLPs can start while the FPS chain and ball
 * lists of levels 1-3 are still being computed (on another stream): gp_encoder_geometry_levels fills the
 * geometry of levels [first, last) (first > 0 reads level first-1's centroids from the workspace);
 * gp_encoder_forward_geom_levels runs SA levels [first, last) of 5 (level l reads level l-1's features from
 * `workspace`; level 4 writes `feat`). geometry_levels(0, 4) == gp_encoder_geometry and
 * forward_geom_levels(0, 5) == gp_encoder_forward_geom; any split gives the same bits. */
int gp_encoder_geometry_levels(const float *pts, int b, int n, void *workspace, size_t workspace_bytes,
                               int first, int last, hipStream_t stream);
int gp_encoder_forward_geom_levels(const float *wbuf, const int64_t *layer_off, const float *pts, int b, int n,
                                   const void *geometry, void *workspace, size_t workspace_bytes, float *feat,
                                   int first, int last, hipStream_t stream);
/* Level-by-level form (the fused encoders, whose levels take features computed between levels):
 * gp_encoder_fps runs the FPS chain of all four levels into the workspace (fps idx + new_xyz, as
 * gp_encoder_workspace_layout places them); gp_sa_level then runs SA level `level`
 * (PointnetSAModuleMSG.forward, pointnet2_modules.py:19-124: ball query of both radii, group, the
 * BN-folded SharedMLPs, max-pool) on its input features feat_prev (b, n_prev, c_prev) point-major
 * (NULL with c_prev = 0 at level 0) -> out (b, M_level, C_level) point-major (level 4: (b, 1024)).
 * c_prev: level 0 any multiple of 16 (Pointnet2ClsMSGFus: 384, pointnet2.py:281-285), level l > 0
 * the previous level's channels. `wbuf`/`layer_off` as gp_encoder_forward, packed for those widths. */
int gp_encoder_fps(const float *pts, int b, int n, void *workspace, size_t workspace_bytes,
                   hipStream_t stream);
int gp_sa_level(const float *wbuf, const int64_t *layer_off, int level, int c_prev, const float *pts,
                int b, int n, const float *feat_prev, void *workspace, size_t workspace_bytes,
                float *out, hipStream_t stream);
/* gp_sa_level over geometry that gp_encoder_geometry left in `geometry` (a workspace of the same (b, n) layout,
 * possibly `workspace` itself): no ball query; the level's scratch goes to `workspace`. The ScoreNet and
 * EnergyNet fused encoders of one batch share one geometry pass this way. Same bits as gp_sa_level. */
int gp_sa_level_geom(const float *wbuf, const int64_t *layer_off, int level, int c_prev, const float *pts,
                     int b, int n, const float *feat_prev, const void *geometry, void *workspace,
                     size_t workspace_bytes, float *out, hipStream_t stream);

/* ===================================================================== fused-encoder blocks
 * The DINO-pointwise encoder Pointnet2ClsMSGFus (pointnet2.py:255-388) between SA levels:
 * TransformerBlockWithRelativePE (attention.py:491-533) with the EfficientRelativePositionalEncoding
 * bias (attention.py:648-735), and GatedAttentionFusion (attention.py:224-325). Token tensors are
 * point-major (b, n, C) fp32, i.e. the reference's (b, C, n) transposed. */
/* y[r, :] = act(x[r, :k] . w^T + bias), r < m; w (n, k) row-major (nn.Linear / Conv1d k=1 layout),
 * k and n multiples of 16; ldx / ldy = row strides of x / y (>= k / n). act: 0 none, 1 ReLU,
 * 2 sigmoid. Exact fp32 MFMA (v_mfma_f32_16x16x4_f32). */
int gp_linear(const float *x, int ldx, int m, int k, const float *w, const float *bias, int n,
              int act, float *y, int ldy, hipStream_t stream);
/* The same linear in split-f16 arithmetic (three v_mfma_f32_16x16x32_f16 products of hi / lo f16
 * planes, fp32 accumulation; x scaled per row by a power of two from its max |x|). wpk: int32 words
 * [e, 0, 0, 0] + the planes of W * 2^e, rows zero-padded to a multiple of 128, in
 * genpose2_amd/fus_encoder.py pack_split_linear's layout (gp_linear_split_words(n, k) words).
 * k % 32 == 0, n % 16 == 0. rmax: m floats, x's row maxima max_k |x| -- computed here, or given
 * by the caller with flags |= GP_LINEAR_RMAX_GIVEN (e.g. the ymax of the linear that produced x).
 * ymax: NULL, or m floats that receive max |y| per row. act 3 is GatedAttentionFusion's gate with its
 * mix (attention.py:316-320): x = [cur | att] (k = 2n), y = g * cur + (1 - g) * att with
 * g = sigmoid(x W^T + b). act 4 adds into y (y += x W^T + b: a residual stream updated in place). act 5 is
 * SwiGLU over output tiles paired (2t, 2t + 1) = (gate, up): y (m, n / 2) with
 * y[:, 16t + c] = silu(z[:, 32t + c]) * z[:, 32t + 16 + c], z = x W^T + b; n % 32 == 0, ldy >= n / 2; ymax is y's. */
#define GP_LINEAR_RMAX_GIVEN 1
size_t gp_linear_split_words(int n, int k);
int gp_linear_split(const float *x, int ldx, int m, int k, const int32_t *wpk, const float *bias, int n,
                    int act, float *y, int ldy, float *rmax, int flags, float *ymax, hipStream_t stream);
/* y = LayerNorm(x + r) over the last dim d (gamma, beta, eps; d % 4 == 0), m rows; y may alias x.
 * ymax: NULL, or m floats that receive max |y| per row. */
int gp_add_layernorm(const float *x, const float *r, int m, int d, const float *gamma,
                     const float *beta, float eps, float *y, float *ymax, hipStream_t stream);
/* Relative-PE bias of EfficientRelativePositionalEncoding (8 heads): xyz (b, n, 3) ->
 * bias (b, 8, n, n) = the reference's relative_bias[b, h, i, j] (query i, key j,
 * rel = xyz[j] - xyz[i]). pe (host-packed, 1024 floats):
 * [0:16) dist.0.w, [16:32) dist.0.b, [32:160) dist.2.w (8x16), [160:168) dist.2.b,
 * [168:216) dir.0.w (16x3), [216:232) dir.0.b, [232:360) dir.2.w, [360:368) dir.2.b,
 * [368:496) fusion.w (8x16), [496:504) fusion.b; then the fusion layer composed with the second
 * layers: [512:640) A[h][u] = (fusion.w[:, :8] dist.2.w)[h][u], [640:768) B[h][u] likewise with
 * dir.2.w, [768:776) c = fusion.w [dist.2.b; dir.2.b] + fusion.b, [776:824) dir.0.w as [axis][u]. */
size_t gp_relpe_bias_bytes(int b, int n);
int gp_relpe_bias(const float *pe, const float *xyz, int b, int n, float *bias, hipStream_t stream);
/* Multi-head attention with an additive bias (MultiheadAttentionWithRelativePE core,
 * attention.py:436-488, eval): qkv (b, n, 3d) rows [q | k | v] (heads of d/8 channels),
 * bias (b, 8, n, n) [b][h][query][key] as gp_relpe_bias writes it, or NULL ->
 * out (b, n, d) = softmax(q k^T / sqrt(d/8) + bias) v per head. ymax: NULL, or b * n floats that
 * receive max |out| per token. */
int gp_mha_attention(const float *qkv, const float *bias, int b, int n, int d, float *out,
                     float *ymax, hipStream_t stream);
/* gp_relpe_bias + gp_mha_attention in one kernel, the bias evaluated per (query, key) pair in registers
 * (no (b, 8, n, n) buffer): qkv as gp_mha_attention, xyz (b, n, 3), pe as gp_relpe_bias. Head dims
 * d / 8 <= 32 (the fused encoder's levels 0 and 1). ymax: NULL or b * n floats (max |out| per token). */
int gp_mha_relpe_attention(const float *qkv, const float *xyz, const float *pe, int b, int n, int d,
                           float *out, float *ymax, hipStream_t stream);
/* F.interpolate(mode="linear", align_corners=False) along the point index: x (b, n_in, c) ->
 * y (b, n_out, c) (pointnet2.py:344-350); c % 4 == 0. ymax: NULL, or b * n_out floats (max |y| per row). */
int gp_interp_points(const float *x, int b, int n_in, int c, int n_out, float *y, float *ymax,
                     hipStream_t stream);
/* GatedAttentionFusion's attention stage (attention.py:298-313) per object: cur (b, n, c), ot (b, n, c)
 * (original_transform output) -> gcat (b, n, 2c) = [cur | ot * ca * sp] with ca = channel attention
 * of mean_n [cur | ot] (ca1: (2c/4, 2c) + bias, ReLU, ca3: (c, 2c/4) + bias, sigmoid) and sp =
 * sigmoid(conv1d_7([max_c cur ; mean_c cur])) (sp_w: (2, 7), zero padding 3). c % 32 == 0.
 * ws: gp_fusion_attend_workspace_size(b, n, c) bytes of device scratch (the per-object statistics).
 * gmax: NULL, or b * n floats that receive max |gcat| per token. */
size_t gp_fusion_attend_workspace_size(int b, int n, int c);
int gp_fusion_attend(const float *cur, const float *ot, int b, int n, int c, const float *ca1_w,
                     const float *ca1_b, const float *ca3_w, const float *ca3_b, const float *sp_w,
                     float *gcat, float *gmax, void *ws, size_t ws_bytes, hipStream_t stream);
/* fused = g * cur + (1 - g) * att with cur = gcat[:, :c], att = gcat[:, c:] (attention.py:318-320):
 * g (rows, c), gcat (rows, 2c) -> out (rows, c). */
int gp_fusion_mix(const float *g, const float *gcat, int rows, int c, float *out, hipStream_t stream);

/* ===================================================================== score / energy heads
 * PoseScoreNet / PoseEnergyNet with Rx_Ry_and_T heads (scorenet.py:109-275, energynet.py:32-208),
 * split into per-object (pts), per-step (t) and per-candidate (pose) column blocks of the first
 * head layer. All "packed" tensors come from genpose2_amd/pack.py. */
typedef struct {
    const float *pe0_w; /* pose_encoder.0: packed 256x16 */
    const float *pe0_b; /* 256 */
    const float *pe2_w; /* pose_encoder.2: packed 256x256 */
    const float *pe2_b; /* 256 */
    const float *h1p_w; /* head layer 1, pose columns: packed 768x256 */
    const float *h2_w;  /* head layer 2: [3 heads][3][256] */
    const float *h2_b;  /* [9] */
    const float *h1pts_t; /* head layer 1, pts columns, transposed (1024, 768) */
    const float *h1_b;    /* head layer 1 bias (768) */
    const float *gfp_w;   /* t_encoder.0.W (64) */
    const float *te_w_t;  /* t_encoder.1.weight transposed (128,128) */
    const float *te_b;    /* (128) */
    const float *h1t_t;   /* head layer 1, t columns, transposed (128, 768) */
    /* f16x3 form of pe2_w / h1p_w (pack.py pack_h16_fragments(w, e, 3), ABI 7): three f16 planes
     * hi, mid, lo of W * 2^e (6 bytes per weight). hsc = {A0, B0, A2, B2, e_pe2, e_h1p, 0, 0}: max row
     * L1 norm and max |bias| of pose_encoder.0 / .2 (activation bounds) and the two weight exponents.
     * Used by every per-candidate head kernel (PC step, score/energy eval, ODE stages): six f16 MFMA
     * products per 32-deep chunk over three planes of each operand, fp32 accumulation. All three NULL:
     * those GEMMs run in exact fp32 MFMA instead. */
    const void *pe2_h;
    const void *h1p_h;
    const float *hsc;
    /* Hybrid form of the PC step's two GEMMs (additive, trailing: a caller that leaves them zero gets the six
     * f16 products everywhere): OCP e4m3 planes of the f16 planes above (pack.py pack_q8_fragments: w_hi x 2^-7,
     * w_mid x 2^4, w_lo x 2^16, 3 bytes per weight, in the A order of v_mfma_scale_f32_16x16x128_f8f6f4). Both
     * given: gp_pc_sample / gp_pc_sample_global form hi*hi, hi*mid and mid*hi on f16 MFMA and the three
     * products of plane order 2 on block-scaled FP8 MFMA (gp_head.h, X3Q) where they run 64-candidate tiles
     * (rows >= 8193; narrower tiles are bound by the weight stream, which the hybrid form makes 7/6 as long, and
     * measured slower); every other kernel keeps the six f16 products. q8_flags: GP_Q8_EVAL routes gp_score_eval
     * through the trunk gp_pc_sample runs on that many rows, so that it returns the PC step's own score bit for
     * bit (the loaders set it with the planes); GP_Q8_ALL_TILES takes the hybrid form at every tile width. */
    const void *pe2_q;
    const void *h1p_q;
    size_t q8_flags;
} gp_head_weights;
enum { GP_Q8_EVAL = 1, GP_Q8_ALL_TILES = 2 };

/* Per-object projection P[b] = W1_pts . pts_feat[b] + b1 -> pobj (b,768). */
int gp_head_object_proj(const gp_head_weights *w, const float *pts_feat, int b, float *pobj,
                        hipStream_t stream);
/* Per-time projection tproj[k] = W1_t . relu(W_t . GFP(t_k) + b_t) for t (nt) -> (nt,768). */
int gp_head_time_proj(const gp_head_weights *w, const float *t, int nt, float *tproj,
                      hipStream_t stream);

/* Score evaluation s = heads(x, t) / (sigma + 1e-7) for R rows, rows r -> object r / k.
 * `tproj_row` (768) and `sigma` are those of the single time value of this call. */
int gp_score_eval(const gp_head_weights *w, const float *pobj, const float *tproj_row,
                  float sigma, const float *x, int rows, int k, float *score, hipStream_t stream);

/* Score and its directional divergence term in one forward-mode pass (cond_ode_likelihood's
 * divergence_eval, samplers.py:54-68, without a backward pass): score (R,9) as gp_score_eval, and
 * div (R) = sum_o eps[r][o] (J_r eps_r)[o] with J_r = d score_r / d x_r, the Skilling-Hutchinson
 * estimate for the direction eps (R,9). The tangent J eps runs through the same GEMMs next to the
 * primal on shared weight fragments, with the primal's ReLU masks (relu' = 0 at 0). */
int gp_score_div_eval(const gp_head_weights *w, const float *pobj, const float *tproj_row,
                      float sigma, const float *x, const float *eps, int rows, int k, float *score,
                      float *div, hipStream_t stream);

/* Energy (IP / score / identical, decoupled rot-trans): pose rows (R,9) with translation
 * already relative to pts_center -> energy (R,2). t is a single value with its tproj row. */
int gp_energy_eval(const gp_head_weights *w, const float *pobj, const float *tproj_row,
                   float sigma, const float *pose, int rows, int k, float *energy,
                   hipStream_t stream);

/* Energy model as a score model (PoseEnergyNet.forward(return_item='score'), energynet.py:211-233):
 * score = grad_x E with E = sum_o x_o f_o(x) / sigma (IP / score / identical, decoupled_rt=False), i.e.
 * score_o = f_o / sigma + (J_f^T c)_o with the cotangent c = x / sigma: one reverse pass through the
 * pose-dependent layers on the transposed weights below, with the forward pass's ReLU masks (relu' = 0 at 0).
 * Forward and reverse GEMMs are exact fp32 MFMA whatever gp_head_weights' f16x3 fields hold. */
typedef struct {
    const float *pe0_wt; /* packed A fragments of pose_encoder.0^T, 16 x 256 (rows 9..15 zero) */
    const float *pe2_wt; /* ... of pose_encoder.2^T, 256 x 256 */
    const float *h1p_wt; /* ... of (head layer 1 pose block)^T, 256 x 768 */
} gp_head_grad_weights;
size_t gp_head_grad_floats(void); /* 16*256 + 256*256 + 256*768 */
/* HOST: row-major pe0_w (256,9), pe2_w (256,256), h1_pose (768,256: the three heads' pose columns, head-major)
 * -> out (gp_head_grad_floats()) = pe0_wt | pe2_wt | h1p_wt; byte-identical to pack.pack_heads_grad */
int gp_head_grad_pack(const float *pe0_w, const float *pe2_w, const float *h1_pose, float *out);
/* score (R,9) = grad_x of sum_o x_o f_o / sigma; energy: NULL or (R) that scalar (return_item
 * 'score_and_energy'). Rows r -> object r / k; a row's result does not depend on the rows evaluated with it. */
int gp_energy_score_eval(const gp_head_weights *w, const gp_head_grad_weights *gw, const float *pobj,
                         const float *tproj_row, float sigma, const float *x, int rows, int k,
                         float *score, float *energy, hipStream_t stream);

/* Probe of the hybrid trunk's e4m3 activation-plane conversion (plane 0 hi: x 2^-7, 1 mid: x 2^4, 2 lo: x 2^16):
 * for n f16 bit patterns (device), q8 = the bytes the trunk's helper makes (packed f16 converted under the scale),
 * q8_via_f32 = the bytes of v_cvt_pk_fp8_f32((float)v * 2^e); n bytes each (device). Only compares conversions. */
int gp_debug_q8_probe(const uint16_t *f16_bits, int n, int plane, uint8_t *q8, uint8_t *q8_via_f32,
                      hipStream_t stream);

/* Test aid for the fp32 pose tail of the PC step: the last step's tail of gp_pc_sample's update waves on
 * caller-given rows, in their lane layout (16 rows per wave, four lanes per row) and through their device
 * functions: mean (R,9) fp32 -> res (R,9) = [GS of [:6], [6:] + pts_center[r / k]] and q (R,7) = [quaternion wxyz
 * of res, res[6:]]. All DEVICE pointers; mean is not written; pts_center holds ceil(rows / k) centres. */
int gp_debug_pose_tail_f32(const float *mean, int rows, int k, const float *pts_center, float *res, float *q,
                           hipStream_t stream);

/* Test aid for the per-object RK45 controller (gp_ode_sample_object): one launch of its control kernel as the
 * sampler launches it for attempt n, on caller-owned DEVICE buffers. It decides attempt n - 1 of every object from
 * rowsq (nobj * kper: per row, the sum over its 9 entries of (err/scale)^2; read when decide != 0) and prepares
 * attempt n. rec_in / rec_out: nobj controller records of gp_debug_ode_obj_rec_size() (168) bytes each, laid out as
 * doubles t, h_abs, t_old, h, t_new, h_abs_loc, coef[6]; floats t32[6], sig[6]; ints status, active, rejected,
 * nfev, n_acc, pend. init (6, nobj, 768): row [s][b] = pobj[b] + the time row of t32[b][s], written for the objects
 * that run. count: one 64-bit word, zero on entry and on return. dev_status[0], and host_status[n & 3] when
 * host_status (host-mapped memory as the device addresses it) is given, receive 4 n + 1 while any object runs and
 * 4 n + 2 once none does. Not part of the sampler's contract: the sampler does not call it. */
size_t gp_debug_ode_obj_rec_size(void);
int gp_debug_ode_obj_control(const gp_head_weights *w, const float *pobj, const void *rec_in, void *rec_out,
                             const double *rowsq, int decide, int n, double t_bound, double direction, int kper,
                             int nobj, float *init, unsigned long long *count, int *host_status, int *dev_status,
                             hipStream_t stream);

/* Test aid for the per-object likelihood (gp_like_sample_object): one launch of its attempt kernel (the six RK45
 * stages of every active object) as the entry launches it, from host-given records on caller-owned DEVICE buffers.
 * rec: rows / k controller records (gp_debug_ode_obj_control's layout); h, t32[6], sig[6], coef[6], active and pend
 * are read. y, ynew and the seven K slots (kslots: HOST array of device pointers; K_0 given) are 10 rows doubles
 * each, [x (9 rows) | logp (rows)]; rowsq (rows) receives, per row of an active object, the sum over its ten entries
 * of (err/scale)^2 in entry order. scratch: (6 rows / k + 1) * 768 floats. An inactive object's rows are not
 * written. Not part of the likelihood's contract: the entry does not call it. */
int gp_debug_like_obj_attempt(const gp_head_weights *w, const float *pobj, const void *rec, const float *eps_dir,
                              double *y, double *ynew, double *const *kslots, double *rowsq, float *scratch,
                              int rows, int k, int rows_total, double rtol, double atol, hipStream_t stream);

/* ===================================================================== PC sampler
 * cond_pc_sampler (samplers.py:113-177) for R = b*k rows over T steps, fused per step:
 * [finish step i-1: Langevin corrector with the batch-mean score norm, renormalise,
 *  reverse-SDE Euler-Maruyama predictor, Gram-Schmidt] + [score at step i].
 * step_tab (HOST, T x 5 fp32): {t, sigma, g, dt, sqrt_dt} exactly as the reference forms them.
 * x (R,9) holds the initial state (prior sample or init_x) and is overwritten.
 * noise: z1/z2 (T,R,9) injected draws, or both NULL to use device Philox4x32 seeded by `seed`.
 * Outputs: res (R,9) = mean_x of the last step (+pts_center, GS), q (R,7) = [quat_wxyz, trans]
 * (posenet_agent.py:554-556), xs (R,T,9) trajectory or NULL. */
size_t gp_pc_workspace_size(int rows);
/* Candidates per PC-step workgroup gp_pc_sample uses for `rows` (split != 0: head weights carry the
 * f16x3 planes). For accounting only (the per-workgroup weight stream). */
int gp_pc_tile_rows(int rows, int split);
int gp_pc_sample(const gp_head_weights *w, const float *pobj, const float *tproj,
                 const float *step_tab, int steps, float *x, int rows, int k,
                 const float *pts_center, const float *z1, const float *z2, uint64_t seed,
                 float snr, float *res, float *q, float *xs, void *workspace,
                 size_t workspace_bytes, hipStream_t stream);
/* gp_pc_sample with the energy model's score (gp_energy_score_eval's, sigma without the + 1e-7) in place of
 * the ScoreNet's: same arguments, workspace, noise streams and outputs; 16 candidates per workgroup. */
int gp_pc_sample_energy(const gp_head_weights *w, const gp_head_grad_weights *gw, const float *pobj,
                        const float *tproj, const float *step_tab, int steps, float *x, int rows, int k,
                        const float *pts_center, const float *z1, const float *z2, uint64_t seed,
                        float snr, float *res, float *q, float *xs, void *workspace,
                        size_t workspace_bytes, hipStream_t stream);

/* Global-batch PC sampling over shards (SURVEY 8e's optional mode; replaces nothing in the reference,
 * whose single cond_pc_sampler call (samplers.py:113-177) couples every row of the batch through the
 * Langevin grad_norm mean at :143-144). Each shard samples its contiguous block of rows
 * [row_off, row_off + rows) of a batch of rows_total rows with the tiling one call on rows_total rows
 * would use: its workgroups' partial sums of ||s_r|| go to entries [shard * per, shard * per + nwg) of
 * `part` (2 x gp_pc_global_partials(...) floats, zero-filled by the caller, per = that count / shards),
 * and after every scoring launch `exchange(ctx, step, slot, n, stream)` must make the slot's n entries
 * hold every shard's partials (an all-gather of `per`-entry chunks, enqueued on `stream`) before the
 * next launch reads them; grad_norm is their sum (in the fixed order) over rows_total, and the Philox
 * draws are keyed by the global row. With every shard but the last holding shard_rows_max rows, a
 * multiple of the tile (gp_pc_tile_rows(rows_total)), the result equals one gp_pc_sample call on the
 * whole batch bit for bit. exchange returns 0 on success. */
typedef int (*gp_pc_exchange_fn)(void *ctx, int step, float *slot, int n, hipStream_t stream);
int gp_pc_global_partials(int rows_total, int shard_rows_max, int shards, int split);
int gp_pc_sample_global(const gp_head_weights *w, const float *pobj, const float *tproj,
                        const float *step_tab, int steps, float *x, int rows, int k,
                        const float *pts_center, uint64_t seed, float snr, float *res, float *q,
                        float *xs, int rows_total, int row_off, int shard, int shards,
                        int shard_rows_max, float *part, gp_pc_exchange_fn exchange, void *ctx,
                        void *workspace, size_t workspace_bytes, hipStream_t stream);

/* Per-object PC sampling: cond_pc_sampler as the reference runs it when called once per object on that
 * object's k candidates. The Langevin step size of a row comes from the mean score norm of its own object's k
 * rows, gn_b = (sum_{j<k} ||s_{b*k+j}||) / k, in place of the mean over every row of the call; nothing else
 * differs from gp_pc_sample. The order of that sum is a function of j and k alone: four chains c_p, p = 0..3,
 * each adding the rows j = p, p+4, p+8, ... in increasing j from 0, combined as (c0 + c1) + (c2 + c3).
 * rows (this call's, whole objects: a multiple of k) are rows [row_off, row_off + rows) of a batch of rows_total
 * rows (row_off a multiple of k, rows_total >= row_off + rows): rows_total selects the tile class
 * (gp_pc_tile_rows(rows_total, split)), so a slice of a large batch runs the large batch's arithmetic, and the
 * Philox draws are keyed by the global row row_off + r. pobj, x, pts_center, the outputs and injected z1 / z2
 * (T, rows, 9) hold this call's objects and rows only. With the f16x3 planes given the step runs the f16x3 trunk
 * at every tile class (the e4m3 planes are not used).
 * Contract: an object's res, q, x and xs rows are bit-identical for any set of other objects in the call and for
 * any split of a batch into calls, given the same rows_total, the same global row index of its rows (Philox
 * draws; any row_off with injected noise) and the same arithmetic (weights, planes, seed, snr, step_tab).
 * workspace: gp_pc_object_workspace_size(rows) bytes; no allocation in the call. Bad arguments return a status
 * and set gp_last_error() before anything is launched. */
size_t gp_pc_object_workspace_size(int rows);
int gp_pc_sample_object(const gp_head_weights *w, const float *pobj, const float *tproj,
                        const float *step_tab, int steps, float *x, int rows, int k,
                        const float *pts_center, const float *z1, const float *z2, uint64_t seed,
                        float snr, float *res, float *q, float *xs,
                        int rows_total, int row_off,
                        void *workspace, size_t workspace_bytes, hipStream_t stream);

/* The step table of cond_pc_sampler (samplers.py:129-130, sde.py:15-27) for hosts without Python:
 * out (HOST, steps x 5 fp32) = {t, sigma(t), g(t), dt, sqrt(dt)} with t = torch.linspace(1, eps,
 * steps) in float32 (bit-identical to torch's CPU rounding), sigma = f32(0.01) * 5000^t (power
 * correctly rounded; torch's Sleef pow is within 1 ulp of it, so sigma / g within 2 / 3 ulp of
 * sde.py's), g = sigma * f32(sqrt(2 ln 5000)), dt, sqrt(dt) (correctly rounded, torch's within 1 ulp).
 * Replaces genpose2_amd/sde.py pc_step_table; feeds gp_head_time_proj (column 0) and gp_pc_sample. */
int gp_pc_step_table(int steps, float eps, float *out);

/* Standard normals (Philox4x32-10 keyed by seed, counter {row, col/4, stream, 0x5EED}, Box-Muller)
 * -> out (rows, cols). The replacement of torch.randn_like in cond_pc_sampler (samplers.py:147,165):
 * gp_pc_sample with z1 = z2 = NULL draws step j's corrector / predictor noise as streams 2j / 2j+1
 * with cols = 9, identical to gp_randn(seed, 2j (+1), rows, 9, ...). */
int gp_randn(uint64_t seed, uint32_t stream, int rows, int cols, float *out, hipStream_t hs);

/* Quaternion / GS epilogue used by the ODE path: rows (R,9) fp64 -> in-place GS of [:6],
 * + pts_center on [6:], and q (R,7) fp64. */
int gp_pose_epilogue_f64(double *pose, int rows, int k, const float *pts_center, double *q,
                         hipStream_t stream);

/* ===================================================================== ODE sampler
 * cond_ode_sampler (samplers.py:180-258): the probability-flow ODE dx/dt = -0.5 g(t)^2 score
 * integrated by a Dormand-Prince 5(4) pair whose controller restates scipy solve_ivp RK45
 * (samplers.py:226-234; the controller's scalars run on the host, genpose2_amd/ode.py).
 * The state y, the stage derivatives K_0..K_6 and y_new are fp64 (R,9) device arrays; the score
 * model sees float(y) (samplers.py:210) at t32 = float(t) with sigma = sigma(t32) in fp32, and a
 * derivative is K = coef * double(score) with coef = -(0.5 g(t)^2) formed on the host.
 * Every call needs gp_ode_workspace_size(rows) bytes of workspace (time rows + error partials). */
size_t gp_ode_workspace_size(int rows);
/* One right-hand side: kout = coef * score(float(y + (sum_{j<nk} acoef[j] kin[j]) * h), t32).
 * kin (HOST array of nk device pointers) and acoef (HOST, nk) may be NULL when nk == 0. */
int gp_ode_rhs(const gp_head_weights *w, const float *pobj, float t32, float sigma, double coef,
               const double *y, const double *const *kin, const double *acoef, int nk, double h,
               int rows, int k, double *kout, void *workspace, size_t workspace_bytes,
               hipStream_t stream);
/* One attempted step (scipy rk.py rk_step + _estimate_error_norm): for s = 1..5
 * K_s = f(t_s, y + (sum_{j<s} A[s][j] K_j) h); y_new = y + (sum_{j<6} B_j K_j) h;
 * K_6 = f(t + h, y_new); err_out[0] = rms((sum_j E_j K_j) h / (atol + max(|y|,|y_new|) rtol)).
 * t32_6 / sigma_6 / coef_6 (HOST, 6 each): stage times 1..5 and t + h. kslots (HOST, 7 device
 * pointers) holds K_0 = f(t, y) on entry. tableau_a (HOST 6x6 row-major), b (HOST 6), e (HOST 7). */
int gp_ode_attempt(const gp_head_weights *w, const float *pobj, const float *t32_6,
                   const float *sigma_6, const double *coef_6, const double *y,
                   double *const *kslots, const double *tableau_a, const double *b, const double *e,
                   double h, double rtol, double atol, int rows, int k, double *ynew, double *err_out,
                   void *workspace, size_t workspace_bytes, hipStream_t stream);
/* select_initial_step norms (scipy _ivp/common.py) over n elements, scale = atol + |y0| rtol:
 * f1 == NULL -> out[0] = rms(y0/scale), out[1] = rms(f0/scale); else out[2] = rms((f1-f0)/scale). */
int gp_ode_init_norms(const double *y0, const double *f0, const double *f1, long long n,
                      double atol, double rtol, double *out, hipStream_t stream);
/* Pose log-likelihood (cond_ode_likelihood, samplers.py:25-110): the same ODE over the augmented
 * state y = [x.reshape(-1) (9R) | logp (R)] (scipy's flat layout), d logp_r / dt = coef * div_r with
 * div of gp_score_div_eval for the constant direction eps (R,9) fp32 and the same coef as x (the VE
 * drift is 0). y, K_0..K_6 and y_new are fp64 arrays of 10 R entries; error norms run over all 10 R
 * (gp_ode_init_norms with n = 10 R serves select_initial_step). gp_like_rhs / gp_like_attempt take
 * the arguments of gp_ode_rhs / gp_ode_attempt plus eps, and need gp_like_workspace_size(rows)
 * bytes of workspace. */
size_t gp_like_workspace_size(int rows);
int gp_like_rhs(const gp_head_weights *w, const float *pobj, float t32, float sigma, double coef,
                const double *y, const float *eps, const double *const *kin, const double *acoef,
                int nk, double h, int rows, int k, double *kout, void *workspace,
                size_t workspace_bytes, hipStream_t stream);
int gp_like_attempt(const gp_head_weights *w, const float *pobj, const float *t32_6,
                    const float *sigma_6, const double *coef_6, const double *y, const float *eps,
                    double *const *kslots, const double *tableau_a, const double *b, const double *e,
                    double h, double rtol, double atol, int rows, int k, double *ynew,
                    double *err_out, void *workspace, size_t workspace_bytes, hipStream_t stream);
/* Per-object likelihood: cond_ode_likelihood as the reference runs it when called once per object on that
 * object's k poses. Every object has its own solve_ivp(RK45) over [x_b (9 k) | logp_b (k)] from t0 to t_bound: its
 * own select_initial_step, step controller, stage times, accept / reject and nfev, and RMS norms over its own 10 k
 * entries (the host-controlled solve over gp_like_attempt takes them over every row of the call). A norm's sum is
 * taken per row over its ten entries in entry order (nine x, then logp), then over the object's rows j < k in an
 * order that is a function of j and k alone (gp_ode_sample_object's). x (rows,9) fp32: the poses the model sees
 * (pts_center subtracted); eps_dir (rows,9) fp32: the Skilling-Hutchinson direction, constant over the solve. rows
 * (whole objects: a multiple of k) are a slice of a batch of rows_total rows (whole objects, >= rows): rows_total
 * selects the tile class (one primal and one tangent tile per workgroup; two pairs from 4,097 rows with the f16x3
 * trunk). pobj, x, eps_dir and the outputs hold this call's objects and rows only.
 * DEVICE outs: z (rows,9) fp64, the latent res.y[:9 k, -1] of every object, and ll (rows) fp64,
 * (prior_logp(z) + delta_logp) / ln 2 with the reference's float32 sigma_max and log term (samplers.py:14-22,
 * 100-109). HOST outs, one per object (rows / k): nfev (2 + 6 attempts), status (1 done, -1 step size below the
 * spacing of t: the object keeps its last state, as the reference does, and the others go on). A finished or
 * failed object is not written again while the others go on; the call runs as many attempts as its slowest object.
 * Contract: an object's ll, z, nfev and status are bit-identical for any set of other objects in the call and for
 * any split of a batch into calls, given the same rows_total, x and eps_dir rows, weights and arithmetic, t0,
 * t_bound, rtol and atol. No exchange between ranks.
 * Workspace: gp_like_object_workspace_size_k(rows, k) bytes (0 when rows are not whole objects);
 * gp_like_object_workspace_size(rows) is enough for every k. Status reads, their 60 s poll limit, the
 * GENPOSE2_ODE_ZC=0 event-and-copy form and the limit of 100,000 attempts are gp_ode_sample_object's: a stuck
 * solve returns an error. Bad arguments (rows that are not whole objects, a rows_total smaller than the call or not
 * whole objects, t0 == t_bound, a workspace that is too small, a null pointer) return a status and set
 * gp_last_error() before anything is launched. */
size_t gp_like_object_workspace_size(int rows);
size_t gp_like_object_workspace_size_k(int rows, int k);
int gp_like_sample_object(const gp_head_weights *w, const float *pobj, const float *x, const float *eps_dir,
                          int rows, int k, int rows_total, double t0, double t_bound, double rtol, double atol,
                          double *z, double *ll, int *nfev, int *status, void *workspace,
                          size_t workspace_bytes, hipStream_t stream);
/* Dense output of an accepted step (scipy RkDenseOutput): for i in [i0, i1),
 * x = (t_eval[i] - t_old)/h, out[row] = h * (K^T P) cumprod([x,x,x,x]) + y_old with
 * row = reverse ? i_base - i : i - i_base. P7x4 (HOST 7x4), kslots (HOST, 7 device pointers). */
int gp_ode_dense(const double *const *kslots, const double *P7x4, const double *y_old,
                 const double *t_eval, int i0, int i1, int i_base, int reverse, double t_old,
                 double h, long long n, double *out, hipStream_t stream);
/* Device-controlled RK45 (the default pred_func path): the step controller itself runs on the
 * device. gp_ode_auto_attempt(n, what): what & 1 launches the control kernel of attempt n -- it
 * decides attempt n-1 from its error norm (scipy _step_impl accept/reject and step-size update)
 * and prepares attempt n (min_step check, h, t_new, the 6 stage times with their scalars and time
 * rows); what & 2 launches attempt n's 6 stage kernels, which return at once if no attempt was
 * prepared. State: two OdeCtl records (gp_ode_ctl_size() bytes each, layout mirrored in
 * genpose2_amd/ode.py) at the start of the workspace; attempt n reads record n & 1 and writes
 * record (n + 1) & 1 (the host writes record 0 after select_initial_step). The status field of a
 * record reads 0 running, 1 finished, -1 step size below the spacing of t. y0/y1: the two fp64
 * state buffers; kslots (HOST, 7 device pointers), tableau_a (HOST 6x6), b (HOST 6), e (HOST 7). */
size_t gp_ode_ctl_size(void);
size_t gp_ode_auto_workspace_size(int rows);
int gp_ode_auto_attempt(const gp_head_weights *w, const float *pobj, int n, int what,
                        double t_bound, double direction, double rtol, double atol,
                        double sig_min, double base, double diff_scale, double *y0, double *y1,
                        double *const *kslots, const double *tableau_a, const double *b,
                        const double *e, int rows, int k, void *workspace, size_t workspace_bytes,
                        hipStream_t stream);
/* gp_ode_auto_attempt whose control kernel also reports to the host without a copy: host_status (4 ints of
 * host memory the device can write, e.g. hipHostMalloc'd) word n & 3 becomes 4 n + (status + 1) once attempt n
 * is decided and prepared, so the host can keep attempts enqueued and poll, with no event or copy between a
 * control launch and its stage launch. */
int gp_ode_auto_attempt_hs(const gp_head_weights *w, const float *pobj, int n, int what,
                           double t_bound, double direction, double rtol, double atol,
                           double sig_min, double base, double diff_scale, double *y0, double *y1,
                           double *const *kslots, const double *tableau_a, const double *b,
                           const double *e, int rows, int k, void *workspace, size_t workspace_bytes,
                           int *host_status, hipStream_t stream);
/* Global-batch RK45 over shards (SURVEY 8e's optional mode for the ODE; replaces nothing in the reference,
 * whose single solve_ivp call (samplers.py:226-234) takes one error norm over the whole batch's state per
 * attempt). Each shard integrates its contiguous rows [row_off, row_off + rows) of rows_total with the
 * tiling of one call on rows_total rows: its workgroups' error partials go to entries
 * [shard * per, shard * per + nwg) of the workspace's gp_ode_global_partials(...) partials (per = that
 * count / shards), and after each attempt's stage launch `exchange(ctx, attempt, part, n, stream)` must
 * make all n entries hold every shard's partials (an all-gather of `per`-entry fp64 chunks enqueued on
 * `stream`) before the next control kernel sums them in the fixed order over rows_total * 9 elements.
 * Every rank then takes the same accept / reject decisions. The caller runs select_initial_step on the
 * WHOLE batch's y0, f0 and f1 (gp_ode_init_norms over all rows_total rows, e.g. after all-gathering the
 * shards' vectors). With every shard but the last holding shard_rows_max rows, a multiple of the tile, the
 * result equals one solve on the whole batch bit for bit. Workspace: gp_ode_global_workspace_size(n)
 * bytes; host_status as gp_ode_auto_attempt_hs, or NULL. */
typedef int (*gp_ode_exchange_fn)(void *ctx, int attempt, double *part, int n, hipStream_t stream);
int gp_ode_global_partials(int rows_total, int shard_rows_max, int shards, int split);
size_t gp_ode_global_workspace_size(int part_n);
/* Byte offset of the error partials (fp64) in a device-controlled workspace: a global-batch host zero-fills
 * the gp_ode_global_partials(...) entries there before the first attempt and all-gathers them in exchange. */
size_t gp_ode_auto_partials_offset(void);
int gp_ode_auto_attempt_global(const gp_head_weights *w, const float *pobj, int n, int what,
                               double t_bound, double direction, double rtol, double atol,
                               double sig_min, double base, double diff_scale, double *y0, double *y1,
                               double *const *kslots, const double *tableau_a, const double *b,
                               const double *e, int rows, int k, int rows_total, int row_off, int shard,
                               int shards, int shard_rows_max, gp_ode_exchange_fn exchange, void *ctx,
                               void *workspace, size_t workspace_bytes, int *host_status,
                               hipStream_t stream);
/* The whole ODE sampler in one call (cond_ode_sampler, samplers.py:180-258, with scipy solve_ivp
 * RK45, samplers.py:226-234) for hosts without Python: x0 (R,9) fp32 device = the prior sample
 * [+ init_x] at T0; select_initial_step on the host from two RHS norms, then device-controlled
 * attempts (gp_ode_auto_attempt), the dense output at eps when steps > 0 (t_eval = linspace(T0, eps,
 * steps); steps = 0: t_eval unset), the final denoise and epilogue (gp_ode_denoise) -> pose (R,9),
 * q (R,7) fp64 device. HOST outs: nfev (scipy's count, including the two select_initial_step
 * evaluations), status (1 done, -1 step size below the spacing of t: with steps > 0 that returns an
 * error, since the t_eval outputs collected before the failure need the host controller).
 * Workspace: gp_ode_sample_workspace_size(rows) bytes. Synchronises `stream` once per attempt (a
 * 4-byte status read, one attempt kept enqueued ahead). Replaces genpose2_amd/ode.py rk45_device +
 * PoseNet._ode (agent.py). */
size_t gp_ode_sample_workspace_size(int rows);
int gp_ode_sample(const gp_head_weights *w, const float *pobj, const float *x0, int rows, int k,
                  double T0, double eps, int steps, double rtol, double atol,
                  const float *pts_center, double *pose, double *q, int *nfev, int *status,
                  void *workspace, size_t workspace_bytes, hipStream_t stream);
/* Per-object ODE sampling: cond_ode_sampler as the reference runs it when called once per object on that
 * object's k candidates. Every object has its own solve_ivp(RK45): its own select_initial_step, step controller,
 * stage times, accept / reject and RMS norms over its k * 9 elements (gp_ode_sample takes them over every row of
 * the call). A norm's sum is taken per row over its 9 entries in increasing order, then over the object's rows
 * j < k in an order that is a function of j and k alone (lane j % 64 of a wave adds its rows in increasing j, the
 * lanes meet in an xor tree). rows (whole objects: a multiple of k) are a slice of a batch of rows_total rows
 * (whole objects, >= rows): rows_total selects the tile class (gp_pc_tile_rows(rows_total, split)). pobj, x0,
 * pts_center and the outputs hold this call's objects and rows only.
 * HOST outs, one per object (rows / k; either may be NULL): nfev (2 + 6 attempts), status (1 done, -1 step size
 * below the spacing of t; with steps > 0 any failed object returns an error, as gp_ode_sample does). A finished or
 * failed object is not written again while the others go on; the call runs as many attempts as its slowest object.
 * Contract: an object's pose, q, nfev, accepted steps and status are bit-identical for any set of other objects in
 * the call and for any split of a batch into calls, given the same rows_total, x0 rows, weights and arithmetic,
 * T0, eps, steps, rtol and atol. No exchange between ranks.
 * Workspace: gp_ode_object_workspace_size_k(rows, k) bytes (six 768-rows per object and attempt);
 * gp_ode_object_workspace_size(rows) is enough for every k. Status reads as gp_ode_sample: host-mapped words the
 * device writes once per attempt (running or not, never one read per object), or an event and a 4-byte copy when
 * the words cannot be mapped or GENPOSE2_ODE_ZC=0. Bad arguments return a status and set gp_last_error() before
 * anything is launched. */
size_t gp_ode_object_workspace_size(int rows);
size_t gp_ode_object_workspace_size_k(int rows, int k);
int gp_ode_sample_object(const gp_head_weights *w, const float *pobj, const float *x0, int rows, int k,
                         int rows_total, double T0, double eps, int steps, double rtol, double atol,
                         const float *pts_center, double *pose, double *q, int *nfev, int *status,
                         void *workspace, size_t workspace_bytes, hipStream_t stream);
/* Final denoise (samplers.py:240-249) + epilogue: grad = score(float(x), t32) fp32,
 * x + (0 - g2 * grad) * step (fp32 product, fp64 sum), GS of [:6], + pts_center, quaternion
 * (posenet_agent.py:554-556) -> pose (R,9) fp64, q (R,7) fp64. */
int gp_ode_denoise(const gp_head_weights *w, const float *pobj, float t32, float sigma, float g2,
                   float step, const double *x, int rows, int k, const float *pts_center,
                   double *pose, double *q, void *workspace, size_t workspace_bytes,
                   hipStream_t stream);
/* The ODE sampler for the energy agent: cond_ode_sampler calls score_model(data) whichever agent it samples
 * (samplers.py:204-219), and PoseEnergyNet answers with grad_x E, E = sum_o x_o f_o(x) / sigma
 * (energynet.py:211-233). Each entry takes the arguments of its namesake plus gw, the transposed weights of the
 * reverse pass (gp_head_grad_weights, as gp_energy_score_eval), and does what its namesake does with that score
 * in place of f / (sigma + 1e-7): a stage's score equals gp_energy_score_eval on float(y_in) at the stage's time
 * row and sigma bit for bit (plain sigma, which must be positive). Exact fp32 on 16-row tiles whatever
 * arithmetic w selects. The stage combination, K = coef * double(score), y_new, the error terms and their fixed
 * summation order, the controller, the dense output and the select_initial_step norms are the score path's own
 * (gp_ode_init_norms, gp_ode_dense and the controller records serve both agents).
 * Workspaces: the existing sizes suffice and are reused -- gp_ode_workspace_size(rows) for gp_ode_rhs_energy,
 * gp_ode_attempt_energy and gp_ode_denoise_energy (one error partial per 16 rows is this tiling's count),
 * gp_ode_auto_workspace_size(rows) for gp_ode_auto_attempt_energy, gp_ode_sample_workspace_size(rows) for
 * gp_ode_sample_energy. gp_ode_auto_attempt_energy takes the host_status of gp_ode_auto_attempt_hs, which may
 * be NULL here (no report to the host). Per-object and global-batch coupling have no energy form.
 * Bad arguments (a NULL gw or gw plane included) return a status and set gp_last_error() before anything is
 * launched. */
int gp_ode_rhs_energy(const gp_head_weights *w, const gp_head_grad_weights *gw, const float *pobj,
                      float t32, float sigma, double coef, const double *y, const double *const *kin,
                      const double *acoef, int nk, double h, int rows, int k, double *kout,
                      void *workspace, size_t workspace_bytes, hipStream_t stream);
int gp_ode_attempt_energy(const gp_head_weights *w, const gp_head_grad_weights *gw, const float *pobj,
                          const float *t32_6, const float *sigma_6, const double *coef_6,
                          const double *y, double *const *kslots, const double *tableau_a,
                          const double *b, const double *e, double h, double rtol, double atol, int rows,
                          int k, double *ynew, double *err_out, void *workspace, size_t workspace_bytes,
                          hipStream_t stream);
int gp_ode_auto_attempt_energy(const gp_head_weights *w, const gp_head_grad_weights *gw, const float *pobj,
                               int n, int what, double t_bound, double direction, double rtol,
                               double atol, double sig_min, double base, double diff_scale, double *y0,
                               double *y1, double *const *kslots, const double *tableau_a,
                               const double *b, const double *e, int rows, int k, void *workspace,
                               size_t workspace_bytes, int *host_status, hipStream_t stream);
int gp_ode_denoise_energy(const gp_head_weights *w, const gp_head_grad_weights *gw, const float *pobj,
                          float t32, float sigma, float g2, float step, const double *x, int rows, int k,
                          const float *pts_center, double *pose, double *q, void *workspace,
                          size_t workspace_bytes, hipStream_t stream);
int gp_ode_sample_energy(const gp_head_weights *w, const gp_head_grad_weights *gw, const float *pobj,
                         const float *x0, int rows, int k, double T0, double eps, int steps, double rtol,
                         double atol, const float *pts_center, double *pose, double *q, int *nfev,
                         int *status, void *workspace, size_t workspace_bytes, hipStream_t stream);

/* ===================================================================== ImgEncoder (--dino pointwise)
 * ImgEncoder.forward (networks/img_encoder/img_encoder.py:48-100) over the three DINOv3 intermediate
 * layers l0, l1, l2 (b, np, d), patch-major as get_intermediate_layers(n=[2, 6, 11], norm=True) returns
 * them (np = g*g patches, d = 384): layer attention (la_w1 (d/2, d), la_b1, la_w2 (d/2), la_b2 a host
 * scalar), geometric attention with the (np, np) position table geo_table (gp_img_geo_table), the 3x3
 * edge conv (conv_w (d/4, d, 3, 3) as stored, conv_b), and the final mix with geo_gate =
 * relu(geo_weight), edge_gate = relu(edge_weight) (host scalars) -> out (b, np, d). Optional outputs
 * (NULL to skip): layer_w (b*np, 3) layer-attention weights, edge_out (b, d/4) edge weights.
 * Workspace: gp_img_encoder_workspace_size(b, np, d) bytes. */
size_t gp_img_encoder_workspace_size(int b, int np, int d);
int gp_img_encoder(const float *l0, const float *l1, const float *l2, int b, int np, int d,
                   const float *la_w1, const float *la_b1, const float *la_w2, float la_b2,
                   const float *geo_table, const float *conv_w, const float *conv_b, float geo_gate,
                   float edge_gate, float *out, float *layer_w, float *edge_out, void *workspace,
                   size_t workspace_bytes, hipStream_t stream);
/* gp_img_encoder with the layer-attention Linear and the edge conv as split-f16 GEMMs (gp_linear_split's
 * arithmetic): la_w1_h / conv_w_h are those weights in fus_encoder.pack_split_linear's layout (conv_w as its
 * (d/4, 9d) rows); NULL runs that GEMM in exact fp32 (gp_img_encoder passes NULL for both). */
int gp_img_encoder2(const float *l0, const float *l1, const float *l2, int b, int np, int d,
                    const float *la_w1, const float *la_b1, const float *la_w2, float la_b2,
                    const float *geo_table, const float *conv_w, const float *conv_b, float geo_gate,
                    float edge_gate, const int32_t *la_w1_h, const int32_t *conv_w_h, float *out,
                    float *layer_w, float *edge_out, void *workspace, size_t workspace_bytes,
                    hipStream_t stream);
/* gp_img_encoder2 with the edge conv's split-f16 GEMM gathering its im2col rows from the fused feature map
 * itself (implicit GEMM: no (b np, 9d) column buffer, ~906 MB at b = 256, np = 256, d = 384). conv_w_hp are the
 * planes of conv_w in POSITION-major order: fus_encoder.pack_split_linear of conv_w.permute(0, 2, 3, 1) as its
 * (d/4, 9d) rows (k index (ky * 3 + kx) * d + channel). The products are the same, summed in that order: within
 * rounding of gp_img_encoder2. conv_w_hp == NULL runs the edge conv in exact fp32 (as gp_img_encoder2 does).
 * Workspace: gp_img_encoder3_workspace_size(b, np, d, conv_w_hp != NULL). */
size_t gp_img_encoder3_workspace_size(int b, int np, int d, int split_conv);
int gp_img_encoder3(const float *l0, const float *l1, const float *l2, int b, int np, int d,
                    const float *la_w1, const float *la_b1, const float *la_w2, float la_b2,
                    const float *geo_table, const float *conv_w, const float *conv_b, float geo_gate,
                    float edge_gate, const int32_t *la_w1_h, const int32_t *conv_w_hp, float *out,
                    float *layer_w, float *edge_out, void *workspace, size_t workspace_bytes,
                    hipStream_t stream);
/* HOST: the geometric attention's position table rel_pos_emb(rel_pos_idx).sum(-1) (img_encoder.py:
 * 68-76): table[i][j] = sum_k E[clamp((r_j - r_i + g - 1)(2g - 1) + (c_j - c_i + g - 1), 0, num_emb - 1)][k]
 * for patches i, j at (row, col) = (p / g, p % g). rel_pos_emb (num_emb, edim) host -> table (g^2, g^2)
 * host (the sum runs in order; torch's vector sum may differ from it in the last bit). */
int gp_img_geo_table(const float *rel_pos_emb, int num_emb, int edim, int grid, float *table);
/* The patch -> point gather of GFObjectPose.extract_pts_feature (posenet.py:146-192): out[b][i] =
 * feat[b][clamp((xs[b][i] // patch_px) * grid + ys[b][i] // patch_px, 0, np - 1)] (floor division;
 * the reference's patch_px = 14, grid = 16). feat (b, np, d), xs/ys (b, n) int32 -> out (b, n, d). */
int gp_gather_patch_points(const float *feat, int b, int np, int d, const int *xs, const int *ys, int n,
                           int patch_px, int grid, float *out, hipStream_t stream);

/* ===================================================================== DINOv3 ViT-S+/16 backbone
 * get_intermediate_layers(rgb, n=out_layers, reshape=False, norm=True, return_class_token=False) of
 * dinov3_vits16plus: D = 384, 12 blocks, 6 heads of 64, patch 16, 1 cls + 4 storage tokens, SwiGLU hidden 1536,
 * LayerNorm eps 1e-5, RoPE on the patch tokens' q and k. All pointers are device pointers.
 * LayerScale is folded into proj / w3 on the host, the qkv bias carries its mask (genpose2_amd/dino.py
 * pack_dino). w12 is [w1 | w2] interleaved in 16-row tiles: rows 32t..32t+15 = w1 rows 16t.., rows
 * 32t+16..32t+31 = w2 rows 16t.. (gate and up of one hidden unit meet in one lane of the SwiGLU epilogue).
 * *_w: row-major fp32 (read by arith 1); *_h: the same matrix in pack_split_linear's layout (read by arith 0). */
typedef struct {
    const float *ln1_w, *ln1_b;
    const float *qkv_w; /* (1152,384) */
    const float *qkv_b; /* bias * bias_mask */
    const float *proj_w; /* ls1 * W (384,384) */
    const float *proj_b; /* ls1 * b */
    const float *ln2_w, *ln2_b;
    const float *w12_w; /* (3072,384), interleaved */
    const float *w12_b;
    const float *w3_w; /* ls2 * W (384,1536) */
    const float *w3_b; /* ls2 * b */
    const int32_t *qkv_h, *proj_h, *w12_h, *w3_h;
} gp_dino_block;
typedef struct {
    const float *patch_w; /* (384,768), k = c * 256 + ky * 16 + kx */
    const float *patch_b;
    const float *cls_token; /* (384) */
    const float *storage_tokens; /* (4,384) */
    const float *norm_w, *norm_b;
    const float *rope; /* gp_dino_rope_table's output for (rope_hp, rope_wp) */
    int rope_hp, rope_wp;
    gp_dino_block blocks[12];
} gp_dino_weights;
enum { GP_DINO_SPLIT_F16 = 0, GP_DINO_F32 = 1 };
/* Bytes of gp_dino_forward's workspace for b images of h x w pixels: room for one chunk of
 * min(b, max(1, 21760 / tokens)) images (0 for arguments gp_dino_forward rejects). */
size_t gp_dino_workspace_size(int b, int h, int w);
/* The RoPE table of an hp x wp patch grid -> table (hp * wp, 64) device floats, per patch [cos(32) | sin(32)]
 * of the angles [h(16) | w(16)]: 2 pi * (2 (i + 0.5) / hp - 1) / periods[k]. periods_host: 16 HOST floats, or
 * NULL for 100^(k/16). Evaluated in float64 on the host, rounded once, copied synchronously. */
int gp_dino_rope_table(const float *periods_host, int hp, int wp, float *table, hipStream_t stream);
/* rgb (b,3,h,w) -> outs[i] (b, hp * wp, 384) = norm(hidden state after block out_layers[i]) without the 5 prefix
 * tokens, i < n_out; only max(out_layers) + 1 blocks run. h, w multiples of 16, hp * wp <= 1024, b >= 1. The batch
 * is processed in chunks of as many images as the workspace holds (at least gp_dino_workspace_size(1, h, w) bytes;
 * chunking does not change a bit of the result). arith: GP_DINO_SPLIT_F16 (the linears as gp_linear_split) or
 * GP_DINO_F32 (gp_linear); the patch embedding and the attention are exact fp32 MFMA in both. */
int gp_dino_forward(const gp_dino_weights *wt, const float *rgb, int b, int h, int w, int n_out,
                    const int *out_layers, float *const *outs, int arith, void *workspace, size_t workspace_bytes,
                    hipStream_t stream);

/* ===================================================================== ScaleNet
 * ScaleNet.forward (scalenet.py:33-49): axes (b,3,3), pts_feat (b,1024) -> length (b,3). */
typedef struct {
    const float *ae0_w; /* (256,180) */
    const float *ae0_b;
    const float *ae2_w; /* (256,256) */
    const float *ae2_b;
    const float *ft0_w; /* (256,1280) */
    const float *ft0_b;
    const float *ft2_w; /* (3,256) */
    const float *ft2_b;
} gp_scale_weights;
int gp_scale_forward(const gp_scale_weights *w, const float *axes, const float *pts_feat, int b,
                     float *length, hipStream_t stream);

/* ===================================================================== ranking / aggregation
 * sort_poses_by_energy (networks/reward.py:131-155) + aggregate_pose
 * (runners/evaluation_single.py:160-219) for b objects of k candidates, one launch.
 * poses (b,k,9) fp32 [rot6 | trans], energy (b,k,2) fp32 [rot, trans] -> aggregated (b,4,4).
 * retain = int(k * retain_ratio) (1..min(k,128)); clustering != 0 runs DBSCAN(eps, min_samples)
 * on the rows of D = 1 - <q_i,q_j>^2 of the retained quaternions and re-averages the largest
 * cluster (min_samples = int(clustering_minpts * retain) as the reference passes it).
 * sorted_pose (b,k,9) / sorted_energy (b,k,2) may be NULL; when given they receive the
 * reference's sort_poses_by_energy outputs (descending, ties by lower index). */
int gp_rank_aggregate(const float *poses, const float *energy, int b, int k, int retain,
                      int clustering, float eps, int min_samples, float *aggregated,
                      float *sorted_pose, float *sorted_energy, hipStream_t stream);

/* Pose hypotheses: gp_rank_aggregate's arguments and outputs (the same bits), and in the same one
 * launch every DBSCAN cluster of the retained rotations instead of the largest alone. max_modes M
 * is 1..8; prev_rot (b,3,3) may be NULL. With L the number of clusters (0 when clustering == 0),
 * the clusters fill slots in descending member count, ties to the lower label, so slot 0 is the
 * cluster gp_rank_aggregate averages; filled = max(1, min(L, M)); with L = 0 slot 0's members are
 * the whole retained set; slots >= filled are zeros.
 *   mode_pose   (b,M,4,4) f32  R of the members' quaternion average (slot 0: aggregated's R, bit for
 *                              bit), t = mean of the members' own translations
 *   mode_count  (b,M) i32      members
 *   mode_energy (b,M) f32      mean rotation energy of the members
 *   mode_spread (b,M) f32      mean 1 - <q_r, q_mode>^2 over the members (the unit of eps)
 *   n_clusters  (b)   i32      L, not capped by M
 *   noise_count (b)   i32      retained rotations DBSCAN labelled noise (0 when clustering == 0)
 *   nearest     (b)   i32      filled slot maximising <q_m, q_prev>^2, q_prev from prev_rot's first
 *                              two columns (ties to the lower slot); -1 when prev_rot is NULL */
int gp_rank_aggregate_modes(const float *poses, const float *energy, int b, int k, int retain,
                            int clustering, float eps, int min_samples, int max_modes,
                            const float *prev_rot, float *aggregated, float *sorted_pose,
                            float *sorted_energy, float *mode_pose, int *mode_count,
                            float *mode_energy, float *mode_spread, int *n_clusters,
                            int *noise_count, int *nearest, hipStream_t stream);

/* ===================================================================== stage glue
 * process_batch's pts_center (datasets_omni6dpose.py:746-752): out (b,3) = mean over n of
 * pts (b,n,c)[:, :, :3], c >= 3. */
int gp_points_mean(const float *pts, int b, int n, int c, float *out, hipStream_t stream);
/* inference_scale without a ScaleNet checkpoint (runners/evaluation_single.py:233-252):
 * pcl (b,n,c) raw points, pose (b,4,4) aggregated [R t; 0 1] -> length (b,3) =
 * 2 * max_n |R^T (p_n - t)| per axis. */
int gp_bbox_length(const float *pcl, int b, int n, int c, const float *pose, float *length,
                   hipStream_t stream);

/* ===================================================================== RGB-D front end
 * One camera frame -> the per-object batch (datasets/datasets_infer.py InferDataset.get_objects; the rules
 * are in DESIGN.md "RGB-D front end"). depth (h,w) float32 metres, color (h,w,3) uint8, mask (h,w) uint8 with
 * 255 = background and every other value an object id; all on the device, none modified. Call sequence:
 * gp_frame_mask_stats, copy the 256 x 5 statistics to the host, gp_frame_crop_boxes (host), upload ids and
 * boxes, gp_frame_objects and gp_frame_roi_rgb, gp_points_mean; read `count` to reject objects with fewer
 * than 10 valid points.
 *
 * Per mask value v: stats[v] = {count, rmin, rmax, cmin, cmax} (int32 (256,5)); an absent value has
 * {0, h, -1, w, -1}. Integer atomics only: the result does not depend on their order. */
int gp_frame_mask_stats(const uint8_t *mask, int h, int w, int *stats, hipStream_t stream);
/* HOST function (no device work; h, w > 40): the object ids present (ascending, 255 left out) -> ids_out
 * (up to 255) and boxes_out (up to 255 x 3: centre x, centre y, scale of the square crop window, all exact
 * in float32) from a host copy of the statistics; *n_out = their number. The window is get_bbox's
 * (utils/sgpa_utils.py: multiples of 40 pixels, at most min(h,w) - 40, shifted back inside the image), centre
 * and scale are aug_bbox_eval's (utils/datasets_utils.py). */
int gp_frame_crop_boxes(const int *stats_host, int h, int w, int *ids_out, float *boxes_out, int *n_out);
/* Bytes of gp_frame_objects' workspace for b objects and an img_size x img_size crop. */
size_t gp_frame_objects_workspace_size(int b, int img_size);
/* Per object (ids, boxes (b,3) on the device): the crop pixels whose nearest source pixel carries the id and a
 * depth in (0, max_depth], in row-major crop order (list V, count[b] = its length c), n_pts of them sampled
 * (c < n_pts: element j is V[j mod c]; else the n_pts smallest of (Philox4x32-10 word 0 of counter
 * {e, id, 0, 0x53414D50} under key = seed's halves, e) in that order) and back-projected with the given
 * (already scaled) intrinsics, each float32 operation rounded on its own -> pts (b,n_pts,3), roi_xs (crop row)
 * and roi_ys (crop column) (b,n_pts) int32, count (b) int32. n_pts <= 2048, img_size even and >= 14. An object
 * with c = 0 gets zeros. */
int gp_frame_objects(const float *depth, const uint8_t *mask, int h, int w, const int *ids, const float *boxes,
                     int b, int img_size, int n_pts, float fx, float fy, float cx, float cy, float max_depth,
                     uint64_t seed, float *pts, int *roi_xs, int *roi_ys, int *count, void *workspace,
                     size_t workspace_bytes, hipStream_t stream);
/* roi_rgb (b,3,img_size,img_size) float32: the bilinear crop of color (taps outside the image are 0), rounded
 * to a uint8 level as floor(value + 0.5), then (level / 255 - mean) / std with the ImageNet constants. */
int gp_frame_roi_rgb(const uint8_t *color, int h, int w, const float *boxes, int b, int img_size, float *roi_rgb,
                     hipStream_t stream);

/* ---- Several frames per call (DESIGN.md "Several frames per call"). f frames (1..65535) of one size, stacked
 * contiguously on the device: depth (f,h,w) float32, mask (f,h,w) uint8, color (f,h,w,3) uint8. The objects of
 * all frames form one batch of b (0..65535; 0 launches nothing), ordered by (frame, id), both ascending;
 * frame_of (b) int32 on the device names each object's frame. Every output of an object has the bits the
 * single-frame entries give on its frame alone. Call sequence: gp_frames_mask_stats, copy the f x 256 x 5
 * statistics to the host, gp_frame_crop_boxes (host) once per frame on that frame's 256 x 5 slice, upload
 * frame_of, ids and boxes, gp_frames_objects and gp_frames_roi_rgb, gp_points_mean; read `count`.
 *
 * stats (f,256,5) int32: gp_frame_mask_stats' table per frame, in one init and one statistics launch. */
int gp_frames_mask_stats(const uint8_t *mask, int f, int h, int w, int *stats, hipStream_t stream);
/* gp_frame_objects on frame frame_of[i] for object i, in one launch. intr (f,4) float32 {fx, fy, cx, cy} (already
 * scaled; a zero focal length gives non-finite points) and seeds (f,2) uint32 {low, high half of the frame's
 * 64-bit seed} are on the device, so cameras and seeds may differ per frame. The workspace is
 * gp_frame_objects_workspace_size(b, img_size). An object whose frame_of lies outside [0, f) reads no frame: it
 * gets count 0 and zeros. */
int gp_frames_objects(const float *depth, const uint8_t *mask, int f, int h, int w, const int *frame_of,
                      const int *ids, const float *boxes, int b, int img_size, int n_pts, const float *intr,
                      float max_depth, const uint32_t *seeds, float *pts, int *roi_xs, int *roi_ys, int *count,
                      void *workspace, size_t workspace_bytes, hipStream_t stream);
/* gp_frame_roi_rgb on frame frame_of[i] for object i, in one launch (a frame_of outside [0, f): the crop of an
 * image without pixels, level 0). */
int gp_frames_roi_rgb(const uint8_t *color, int f, int h, int w, const int *frame_of, const float *boxes, int b,
                      int img_size, float *roi_rgb, hipStream_t stream);

/* ===================================================================== weight packing
 * The load path of PoseNet.load_ckpt -> load_state_dict (posenet_agent.py:171-203) for the --dino none
 * models, without Python: a model's state-dict tensors (HOST float32 arrays named by the reference's
 * model_state_dict keys; a "module." prefix is stripped; num_batches_tracked and unknown keys are ignored)
 * -> every packed layout the kernels read (BN folded in float64, MFMA fragment order, split-f16 planes and
 * bounds), byte-identical to genpose2_amd/pack.py.
 * gp_weights_pack uploads them into ONE device allocation (the only allocating call of the library; not a
 * hot call) and returns an opaque handle; gp_weights_heads / gp_weights_scale / gp_weights_encoder give
 * the structs and pointers the other entry points take (valid until gp_weights_free).
 * gp_weights_pack_host writes the same packed buffer to host memory instead (out == NULL: size query):
 * fields[GP_PACK_NFIELDS] = float offsets of the encoder buffer (GP_PACK_ENC), the 16 gp_head_weights
 * fields in struct order (GP_PACK_HEADS + i) or the 8 gp_scale_weights fields (GP_PACK_SCALE + i), -1 if
 * absent; enc_table (120 int64) = gp_encoder_forward's layer_off relative to the encoder buffer. */
enum { GP_MODEL_SCORE = 0, GP_MODEL_ENERGY = 1, GP_MODEL_SCALE = 2 };
enum { GP_PACK_ENC = 0, GP_PACK_HEADS = 1, GP_PACK_SCALE = 17, GP_PACK_NFIELDS = 25 };
typedef struct gp_weights gp_weights;
int gp_weights_pack(int kind, int n, const char *const *names, const float *const *data,
                    const int64_t *numel, gp_weights **out);
void gp_weights_free(gp_weights *w);
const gp_head_weights *gp_weights_heads(const gp_weights *w);
const gp_scale_weights *gp_weights_scale(const gp_weights *w);
const float *gp_weights_encoder(const gp_weights *w, const int64_t **layer_off);
int gp_weights_pack_host(int kind, int n, const char *const *names, const float *const *data,
                         const int64_t *numel, float *out, size_t out_floats, size_t *need_floats,
                         int64_t *fields, int64_t *enc_table);

#ifdef __cplusplus
}
#endif
#endif /* GENPOSE_HIP_H */
