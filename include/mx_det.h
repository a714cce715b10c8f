/* mx_det.h — C ABI of libmx_det.so, the MI355X (gfx950) hot path of the Faster R-CNN
 * R50-FPN v2 train/eval step, corruption augmentation and U-Net restoration pre-pass of
 * ysbbin/Robust-Object-Detection.
 *
 * The reference has no plugin API of its own: its hot path is reached through
 * torchvision / OpenCV calls made from its scripts. Each entry point below names the reference call
 * site and the third-party operator it replaces, so a maintainer can bind it (ctypes stub in
 * INTEGRATION.md; the package robust-object-detection_amd/mx_det is that binding).
 *
 * Conventions
 *  - Every pointer argument is a device pointer owned by the caller; the library never allocates
 *    or frees on these paths. Scratch comes from a caller workspace sized by *_workspace().
 *  - Work is enqueued on `stream` (a hipStream_t) and is stream-ordered; nothing synchronises.
 *  - Exceptions, off the hot path and marked at their declarations: the convenience forms
 *    (mx_conv2d_fwd / _dgrad / _wgrad, mx_bn_finalize, mx_bn_bwd_reduce / _apply) allocate their
 *    temporaries with hipMallocAsync / hipFreeAsync on `stream` (the _ex forms take a workspace);
 *    mx_conv_pack_batched with upload = 1 synchronises `stream` once to copy a NEW job plan to the
 *    device (the steady state passes upload = 0 and only launches).
 *  - Return 0 on success, negative MX_E* on error; mx_last_error() gives the message (thread-local).
 *  - Activations are NHWC; conv weights are KRSC (Cout, kh, kw, Cin); dtype codes below.
 */
#ifndef MX_DET_H
#define MX_DET_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MX_OK 0
#define MX_EINVAL -1
#define MX_EUNSUPPORTED -2
#define MX_EHIP -3

#define MX_F32 0
#define MX_BF16 1

typedef void* mx_stream_t; /* hipStream_t */

int mx_version(void);
const char* mx_last_error(void);
/* Launches an empty kernel (trace_marker_kernel) on `stream`: a marker in rocprofv3 kernel traces. */
int mx_trace_marker(int id, mx_stream_t stream);
/* A dedicated non-blocking HIP stream on `device` (never destroyed: the process's side streams). The
 * framework's own streams come from here, not from torch's round-robin pool of 32 streams per device:
 * a process creating more pool streams than that (a model per test, a loader per epoch) would alias
 * two of them -- e.g. a side stream with a graph's capture stream. */
int mx_stream_create(int device, mx_stream_t* out);

/* ---------------------------------------------------------------------------------------------
 * Anchor assignment: torchvision box_iou + Matcher (+ label/target construction), fused.
 * Replaces RegionProposalNetwork.assign_targets_to_anchors / RoIHeads.assign_targets_to_proposals
 * (reached from train_frcnn_baseline.py:171, model(images, targets)).
 *   gt[G,4], boxes[A,4] xyxy f32. matches[A] int64: gt index, -1 below low, -2 between.
 *   mode 0: matches only.
 *   mode 1 (RPN):  labels_f32[A] = 1 / 0 / -1 ; targets[A,4] = encode(gt[max(m,0)], boxes, w)
 *   mode 2 (RoI):  labels_i64[A] = gt_labels[max(m,0)] / 0 (below) / -1 (between); targets as mode 1
 *   G == 0 is allowed (all background, matches = -1, zero targets), as the empty-target path of
 *   coco_detection_dataset.py:44-48 requires.
 * ------------------------------------------------------------------------------------------- */
size_t mx_match_workspace(int64_t G, int64_t A);
int mx_match_assign(const float* gt, const int64_t* gt_labels, int64_t G, const float* boxes, int64_t A,
                    float high, float low, int allow_low_quality, int mode, const float* enc_weights4_host,
                    int64_t* matches, void* labels, float* targets, void* ws, size_t ws_bytes, mx_stream_t stream);

/* The same for B images in one launch (grid.y = image): gt [B][G][4] of which gcount[b] (device int32,
 * nullable = all G) rows are real -- a zero-padded, static-shape GT batch -- gt_labels [B][G]; boxes
 * [B][box_stride rows] (box_stride 0: one [A,4] set shared by every image, the RPN anchors);
 * matches / labels [B][A], targets [B][A][4]; counts (nullable) [B][2] int32 = per image the number of
 * boxes matched (label >= 1) and background (label 0) -- BalancedPositiveNegativeSampler's pos / neg
 * counts without a reduction pass. Workspace mx_match_batched_workspace(B, G, A). */
size_t mx_match_batched_workspace(int64_t B, int64_t G, int64_t A);
int mx_match_assign_batched(const float* gt, const int64_t* gt_labels, const int32_t* gcount, int64_t B, int64_t G,
                            const float* boxes, int64_t box_stride, int64_t A, float high, float low,
                            int allow_low_quality, int mode, const float* enc_weights4_host, int64_t* matches,
                            void* labels, float* targets, int32_t* counts, void* ws, size_t ws_bytes,
                            mx_stream_t stream);

/* torchvision.ops.box_iou -> out[n,m] (test/diagnostic entry). */
int mx_box_iou(const float* b1, int64_t n, const float* b2, int64_t m, float* out, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * NMS: torchvision.ops.nms / batched_nms (boxes.py), CPU semantics: stable score-descending order,
 * suppress when IoU > thr. Replaces RegionProposalNetwork.filter_proposals' batched_nms(level) and
 * RoIHeads.postprocess_detections' batched_nms(label) (eval_all.py:111).
 *   idxs == NULL -> plain nms. mode: 0 = CPU dispatch rule (4*n > 4000 -> per-class, else
 *   coordinate-offset trick), 1 = per-class, 2 = coordinate trick.
 *   group (nullable, int32[n]): output is ordered by (group asc, score desc) instead of score desc,
 *   so several images can share one call.
 *   keep[n] int64 receives kept indices; *num_keep (device int64) the count.
 *   max_seg: upper bound on the number of boxes that share one idx value (n is always safe).
 * ------------------------------------------------------------------------------------------- */
/* One call for all images of RegionProposalNetwork.filter_proposals (torchvision calls batched_nms
 * once per image, rpn.py filter_proposals): box i belongs to image group[i] (entries with
 * group >= G are dead and never kept) and level lvl[i] in [0, L). Per image, the CPU dispatch rule
 * of torchvision.ops.batched_nms is applied on the device: more than 1000 live boxes -> NMS per
 * level, else the coordinate trick with that image's max coordinate. keep[0:num_keep] = survivors
 * ordered by (image, score desc, index); num_keep is written on the device (-1: a segment exceeded
 * max_seg). Workspace from mx_nms_grouped_workspace(n, G, max_seg). */
size_t mx_nms_grouped_workspace(int64_t n, int64_t G, int64_t max_seg);
int mx_batched_nms_grouped(const float* boxes, const float* scores, const int64_t* lvl, const int32_t* group,
                           int64_t n, int64_t G, int64_t L, int64_t max_seg, double iou_threshold, int64_t* keep,
                           int64_t* num_keep, void* ws, size_t ws_bytes, mx_stream_t stream);
/* Presorted form of mx_batched_nms_grouped, same result (bit-identical keep[0:num_keep]) in 4
 * launches instead of ~20 (no radix sorts): meant for filter_proposals' candidates, whose live entries
 * come image-major, level-major, and score-descending within each (image, level) run (the per-level
 * top-k order; a run found out of order is still ranked exactly, by counting). n <= 24576, G <= 64,
 * L <= 8. keep[num_keep:n] is filled with 0. post > 0: also sel [G, post] int64 = per image the first
 * post survivors (0 past the image's count) and valid [G, post] uint8 -- filter_proposals' padded
 * selection. Workspace from mx_nms_grouped_workspace(n, G, max_seg). Replaces the per-image
 * batched_nms of torchvision rpn.py filter_proposals (train_frcnn_baseline.py:171). */
int mx_batched_nms_grouped_sorted(const float* boxes, const float* scores, const int64_t* lvl, const int32_t* group,
                                  int64_t n, int64_t G, int64_t L, int64_t max_seg, double iou_threshold,
                                  int64_t* keep, int64_t* num_keep, int64_t post, int64_t* sel, uint8_t* valid,
                                  void* ws, size_t ws_bytes, mx_stream_t stream);
/* RegionProposalNetwork._get_top_n_idx (torchvision rpn.py:221-233, reached from
 * train_frcnn_baseline.py:171): for each image row of scores [N, row_stride] and each level l
 * (columns level_off[l] .. +level_n[l]), the indices of the min(k, level_n[l]) largest scores,
 * value descending (ties: index ascending; the set at a tied threshold takes the lowest indices),
 * plus level_off[l]; levels concatenated: out_idx [N, sum_l min(k, level_n[l])] int64.
 * 1 <= nlev <= 8, min(k, level_n[l]) <= 4096. */
int mx_level_topk(const float* scores, int64_t N, int64_t row_stride, int nlev, const int64_t* level_off,
                  const int64_t* level_n, int64_t k, int64_t* out_idx, mx_stream_t stream);
/* mx_level_topk with a workspace of mx_level_topk_workspace(N, nlev, level_n) bytes (0: no level is
 * long enough to slice; ws may then be NULL): a level above 24,576 elements is cut into slices whose
 * own top-k lists (in ws) are merged by a second launch -- the same result, read by many CUs.
 * ws == NULL: every level is one workgroup (mx_level_topk). */
size_t mx_level_topk_workspace(int64_t N, int nlev, const int64_t* level_n);
int mx_level_topk_ws(const float* scores, int64_t N, int64_t row_stride, int nlev, const int64_t* level_off,
                     const int64_t* level_n, int64_t k, int64_t* out_idx, void* ws, size_t ws_bytes,
                     mx_stream_t stream);
size_t mx_nms_workspace(int64_t n, int64_t max_seg);
int mx_batched_nms(const float* boxes, const float* scores, const int64_t* idxs, const int32_t* group, int64_t n,
                   int64_t max_seg, double iou_threshold, int mode, int64_t* keep, int64_t* num_keep, void* ws,
                   size_t ws_bytes, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * RoIAlign (torchvision::roi_align / _roi_align_backward, aligned flag honoured), NHWC features.
 * Multi-scale form = MultiScaleRoIAlign(['0'..'3'], 7, 2) with its LevelMapper
 * (floor(4 + log2(sqrt(area)/224) + 1e-6) clamped to [k_min, k_max]) — replaces
 * RoIHeads.box_roi_pool reached from train_frcnn_baseline.py:171 / eval_all.py:111.
 *   feats[l]: NHWC [N, H[l], W[l], C] of dtype; rois[K,5] f32 (batch, x1,y1,x2,y2).
 *   out: [K, PH, PW, C] dtype.  Backward (torchvision _roi_align_backward,
 *   roi_align_kernel.cpp roi_align_backward_kernel_impl): grad_feats[l] NHWC f32 over N images.
 *     deterministic = 1: atomic-free gather -- every element of every grad map is WRITTEN (no
 *       zero-fill needed) with one fixed summation order per element (RoI ascending, bin, corner):
 *       bitwise reproducible run to run. Needs C % 4 == 0 with C <= 256, pooled bins <= 64, sampling <= 4, level maps
 *       < 32768 px a side, and a workspace of mx_roi_align_bwd_workspace(K, PH, PW, sampling) bytes.
 *     deterministic = 0: float atomics ACCUMULATE into caller-zeroed maps (order-dependent in
 *       the last bits; no workspace).
 *   sampling <= 0: torchvision's adaptive grid (the roi_align default sampling_ratio=-1): per RoI,
 *     ceil(roi_h / PH) x ceil(roi_w / PW) samples per bin. Forward bit-exact like the fixed grid;
 *     backward with deterministic = 0 only (atomics, as torchvision's CUDA kernel).
 * ------------------------------------------------------------------------------------------- */
size_t mx_roi_align_bwd_workspace(int64_t K, int PH, int PW, int sampling);
/* deterministic-gather tile width (pixels per wave strip): 2 (default), 4 or 8. Results are identical;
 * 4-wide tiles shorten the tail of tiles that many RoIs overlap. Not thread-safe (a process setting). */
int mx_roi_bwd_set_strip(int sw);
/* forward: channel slices per RoI (1, 2, 4 (default) or 8 when C / 8 divides): more, shorter blocks.
 * A process setting, results identical. */
int mx_roi_fwd_set_split(int n);
int mx_roi_align_fwd(const void* feat, int dtype, int64_t N, int64_t H, int64_t W, int64_t C, const float* rois,
                     int64_t K, float spatial_scale, int PH, int PW, int sampling, int aligned, void* out,
                     mx_stream_t stream);
int mx_roi_align_bwd(const void* grad_out, int dtype, int64_t N, int64_t H, int64_t W, int64_t C, const float* rois,
                     int64_t K, float spatial_scale, int PH, int PW, int sampling, int aligned, float* grad_feat,
                     int deterministic, void* ws, size_t ws_bytes, mx_stream_t stream);
int mx_multiscale_roi_align_fwd(const void* const* feats_host, const int64_t* H_host, const int64_t* W_host,
                                const float* scales_host, int nlev, int k_min, int dtype, int64_t C,
                                const float* rois, int64_t K, int PH, int PW, int sampling, void* out,
                                int32_t* levels_out, mx_stream_t stream);
int mx_multiscale_roi_align_bwd(const void* grad_out, int dtype, float* const* grad_feats_host, int64_t N,
                                const int64_t* H_host, const int64_t* W_host, const float* scales_host, int nlev,
                                int64_t C, const float* rois, const int32_t* levels, int64_t K, int PH, int PW,
                                int sampling, int deterministic, void* ws, size_t ws_bytes, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Anchors and box coder (torchvision AnchorGenerator / BoxCoder, anchor_utils.py, _utils.py).
 * ------------------------------------------------------------------------------------------- */
/* One FPN level: cell anchors round([-ws,-hs,ws,hs]/2) for `size` and ratios, shifted by
 * arange*stride; order (y, x, ratio). out[gh*gw*nr, 4]. */
/* filter_proposals after the per-level top-k (rpn.py): boxes [N*T, 4] = proposals[n][top[n][t]]
 * clipped to (h, w) = hw[n] (clamp(min=0) then minimum, NaN-propagating as torch), grp [N*T] int32 = n
 * when the box is at least min_size wide and high and prob >= score_thresh, else N. top [N, T] int64
 * indices into the A proposals of the image; prob [N, T]; hw [N, 2] (h, w) f32. */
int mx_proposal_clip_filter(const float* proposals, const int64_t* top, const float* prob, const float* hw,
                            int64_t N, int64_t A, int64_t T, float min_size, float score_thresh, float* boxes_out,
                            int32_t* grp_out, mx_stream_t stream);
/* GeneralizedRCNN's degenerate-box check: flag[0] = any box of the m (<= 8) sets (boxes_host[j]:
 * counts_host[j] x 4 f32 on the device, x1 y1 x2 y2) has x2 <= x1 or y2 <= y1; one launch, the flag
 * is always written. */
int mx_boxes_degenerate(const float* const* boxes_host, const int64_t* counts_host, int m, uint8_t* flag,
                        mx_stream_t stream);
/* RoIHeads' sampled-RoI compaction: the K selected entries of mask [M] (bool, M = N x cm
 * candidates, K = their count, known on the host) in ascending order -> rois [K, 5] (entry / cm as
 * f32, then box[entry]), lab_out [K] = lab[entry] (int64), tg_out [K, 4] = tg[entry]. */
int mx_roi_compact(const uint8_t* mask, int64_t M, int64_t K, int64_t cm, const float* box, const int64_t* lab,
                   const float* tg, float* rois, int64_t* lab_out, float* tg_out, mx_stream_t stream);
int mx_anchors_level(float size, const float* ratios_host, int nr, int64_t gh, int64_t gw, int64_t stride_h,
                     int64_t stride_w, float* out, mx_stream_t stream);
/* decode_single: rel[n, ncls*4] against boxes[n,4] -> out[n, ncls*4]; weights (wx,wy,ww,wh);
 * dw/dh clamped at `clip`. */
int mx_box_decode(const float* rel, const float* boxes, int64_t n, int64_t ncls, const float* weights4_host,
                  float clip, float* out, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Detection postprocessing for every image of a batch without a host round trip: torchvision
 * RoIHeads.postprocess_detections (roi_heads.py) + GeneralizedRCNNTransform.postprocess, reached from
 * eval_all.py:111 / eval_restored.py, model(images) in eval mode. Three stream-ordered steps:
 *   mx_det_candidates -> mx_batched_nms_grouped(lvl = labels, L = C, group = grp, G = N) -> mx_det_select
 * ------------------------------------------------------------------------------------------- */
/* Front half, one launch: softmax, box decode, clip to the image, score and small-box filter.
 *   logits [R][ldl] f32, C class columns (column 0 = background), 2 <= C <= 1024, ldl >= C;
 *   reg [R][ldr] f32, 4 values per class, ldr >= 4*C (any strides: rows need no 16-byte alignment);
 *   rois [R][4] f32 xyxy; img [R] int32 = the image of each row (outside [0, N): a padded / dead row);
 *   hw [N][2] f32 (h, w) as mx_proposal_clip_filter; weights4_host / clip as mx_box_decode.
 * For row r and class c in 1..C-1, at the dense index t = r*(C-1) + (c-1) (the order torch's
 * compaction keeps, so ties broken by index downstream break as in the reference):
 *   scores[t] = softmax probability in f32: m = max_j x_j; e_j = expf(x_j - m); s = sum of e_j for
 *     j = 0..C-1 in ascending j; p = e_c / s (IEEE division) -- independent of the launch geometry;
 *   boxes[t]  = mx_box_decode's box (the same device function) with x clamped to [0, w] and y to [0, h]
 *     as torch.clamp does (NaN stays NaN, +-inf goes to the bound); a dead row's box is not clamped;
 *   labels[t] = c (int64);
 *   grp[t]    = img[r] when the row is live, score > score_thresh (strictly) and the clamped width and
 *     height are both >= min_size (comparisons false on NaN), else N (dead).
 * All four outputs are written at every t. R == 0 launches nothing. */
int mx_det_candidates(const float* logits, int64_t ldl, const float* reg, int64_t ldr, const float* rois,
                      const int32_t* img, const float* hw, int64_t R, int64_t C, int64_t N,
                      const float* weights4_host, float clip, float score_thresh, float min_size, float* scores,
                      float* boxes, int64_t* labels, int32_t* grp, mx_stream_t stream);
/* Back half, one launch: keep [>= num_keep] / num_keep (device int64) from mx_batched_nms_grouped over
 * the n = R*(C-1) dense candidates boxes / scores / labels / grp. Per image g < N, with cnt = min(its
 * number of survivors, D) (D = detections_per_img):
 *   out_boxes [N][D][4] = its first cnt survivors in keep order (score descending, ties by index),
 *     x multiplied once by rw and y by rh, ratios [N][2] f32 (rh, rw) on the device; NULL: no rescale;
 *   out_scores [N][D], out_labels [N][D] int64; counts [N] int32 = cnt.
 * Every element of every output is written; slots past cnt are 0. num_keep < 0 (an NMS segment over
 * max_seg) sets every count to -1, so a failed NMS never passes for an empty result. n == 0 is
 * allowed (keep and the candidate arrays may then be NULL). */
int mx_det_select(const int64_t* keep, const int64_t* num_keep, const float* boxes, const float* scores,
                  const int64_t* labels, const int32_t* grp, int64_t n, int64_t N, int64_t D, const float* ratios,
                  float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* counts, mx_stream_t stream);
/* Test-time augmentation: V views of each of N images through the model, their detection sets fused
 * by box voting (Gidaris & Komodakis 2015; Detectron's bbox_vote). The box head ran on V*N*P rows
 * ordered view-major, then image, then row, and mx_det_candidates was called with N' = V*N, so slot
 *   t = ((v*N + i)*P + r)*(C-1) + (c-1),  n = V*N*P*(C-1),  a live slot has grp[t] == v*N + i.
 * Both entries check n == V*N*P*(C-1) < 2^30, 1 <= V <= 64, 2 <= C <= 1024. Stream-ordered chain:
 *   mx_det_candidates(N' = V*N) -> mx_det_views_fold -> mx_batched_nms_grouped(G = N) -> mx_det_select_vote */
/* One elementwise launch that brings every view's candidates into the image's own frame and group.
 * For slot t of block b = v*N + i:
 *   grp[t] == b (live): grp_out[t] = i; when flip_host[v] != 0 (int32 [V] on the host), the box is
 *     mirrored in continuous coordinates as torchvision's horizontal flip maps boxes: x1' = w - x2,
 *     x2' = w - x1 with w = hw[i][1] (hw [N][2] f32 (h, w), the resized sizes), one f32 subtraction
 *     each, y unchanged; candidates are clamped to [0, w], so 0 <= x1' <= x2' <= w;
 *   any other grp[t] (dead): grp_out[t] = N and the box is copied unchanged.
 * Every element of both outputs is written; boxes_out == boxes and grp_out == grp are allowed.
 * n == 0 launches nothing. */
int mx_det_views_fold(const float* boxes, const int32_t* grp, const float* hw, int64_t n, int64_t V, int64_t N,
                      int64_t P, int64_t C, const int32_t* flip_host, float* boxes_out, int32_t* grp_out,
                      mx_stream_t stream);
/* mx_det_select on the folded candidates (outputs, counts, zeros past the count, -1 counts when
 * num_keep < 0, n == 0, ratios: all as there) with each selected survivor's box replaced by the
 * score-weighted mean of its voters, in one launch. For survivor k of image g with label c
 * (1 <= c < C), the voters are the slots t = ((v*N + g)*P + r)*(C-1) + (c-1), v = 0..V-1,
 * r = 0..P-1, with grp[t] == g and iou(box_k, box_t) >= vote_iou (false on NaN), where
 *   iou = inter / ((area_k + area_t) - inter), area = (x2 - x1)*(y2 - y1),
 *   inter = max(min(x2) - max(x1), 0) * max(min(y2) - max(y1), 0)
 * is torchvision's box_iou in f32, every operation rounded once, and vote_iou is rounded to f32 once.
 * Per coordinate the voted value is (float)(sum_t (double)s_t*(double)b_t / sum_t (double)s_t): both
 * sums f64, added in ascending slot order with one rounding per add (each f32 x f32 product is exact
 * in f64), one f64 division, one rounding to f32 -- independent of the launch geometry. A survivor
 * whose only voter is itself keeps its box bit for bit; a voted coordinate lies within its voters'
 * minimum and maximum. A survivor with no voter at all (or a label outside [1, C)) keeps its box.
 * The box is then multiplied once by rw / rh as in mx_det_select; score and label are the survivor's.
 * vote_iou > 1 or NaN: no voting, the output is bitwise mx_det_select's. */
int mx_det_select_vote(const int64_t* keep, const int64_t* num_keep, const float* boxes, const float* scores,
                       const int64_t* labels, const int32_t* grp, int64_t n, int64_t V, int64_t N, int64_t P,
                       int64_t C, int64_t D, double vote_iou, const float* ratios, float* out_boxes,
                       float* out_scores, int64_t* out_labels, int32_t* counts, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Corruption augmentation (scripts/augmentations.py:14-56, RandomCorruption :60-74), uint8 HWC.
 *   op: 0 identity, 1 noise (sigma, Philox seed; or `noise` field f32 if non-NULL), 2 motion blur
 *   (k=9, angle 0), 3 low-res (INTER_AREA x factor, INTER_LINEAR back). Batched form takes one op
 *   per image; images are [B, H, W, 3] contiguous. tmp: >= B*nh*nw*3 bytes for op 3.
 * ------------------------------------------------------------------------------------------- */
int mx_corrupt_u8(const uint8_t* img, int64_t B, int64_t H, int64_t W, int64_t C, const int32_t* ops_host,
                  float sigma, uint64_t seed, const float* noise, double factor, uint8_t* tmp, uint8_t* out,
                  mx_stream_t stream);
/* apply_motion_blur at any kernel size / angle (augmentations.py:21-38): cv2.filter2D(img, -1, kernel)
 * on uint8 [B,H,W,C] with the non-zero taps of the k x k float kernel given as ntaps (dy, dx, coef)
 * triples (row-major kernel order, offsets from the anchor = kernel centre), BORDER_REFLECT_101,
 * f32 sum, round half to even. The kernel itself (getRotationMatrix2D + warpAffine of the centre row,
 * normalised) is built on the host (mx_det.augment.motion_blur_kernel). ntaps <= 128; not in place.
 * Low-res (op 3) takes OpenCV's exact-x2 INTER_AREA fast path when W == 2*nw and H == 2*nh. */
int mx_filter2d_u8(const uint8_t* img, int64_t B, int64_t H, int64_t W, int64_t C, const float* taps_host, int ntaps,
                   uint8_t* out, mx_stream_t stream);
/* The corruptions for a whole batch in one launch, each image with its own op, strength and size
 * (severity sweeps, severity-randomised augmentation, a list of detection frames of any sizes).
 * One descriptor per image, in a host array: */
typedef struct mx_corrupt_desc {
  const uint8_t* src; /* device, u8 [H][W][3] */
  uint8_t* dst;       /* device, u8 [H][W][3] */
  int32_t H, W;       /* 1..32768 each */
  int32_t op;         /* 0 none (copy), 1 noise, 2 blur, 3 low-res */
  float sigma;        /* op 1 */
  uint64_t seed;      /* op 1: Philox key; the counter is the element's flat index within its image */
  int32_t tap_off, ntaps; /* op 2: this image's (dy, dx, coef) triples in the call's tap table; ntaps <= 128,
                             |dy|, |dx| <= 15 */
  int32_t nh, nw;     /* op 3: the low-res size, 1 <= nh <= H, 1 <= nw <= W */
} mx_corrupt_desc;
/* out = the same bits as mx_corrupt_u8 (ops 1, 3; op 3 takes the exact-x2 path when W == 2*nw and
 * H == 2*nh) and mx_filter2d_u8 (op 2, any tap set within the reach) give for that image alone. taps_host:
 * ntaps_total (dy, dx, coef) f32 triples, row-major kernel order, shared by the descriptors. noise: NULL
 * (Philox from sigma / seed), or one f32 field on the device for the whole call: the images' [H][W][3]
 * fields back to back in descriptor order, whatever their ops (for a [B,H,W,3] batch: [B][H][W][3]).
 * One launch per chunk of 16 images (fewer when their distinct tap sets exceed 192 taps); descriptors
 * and taps travel as kernel arguments: no workspace, no upload, no host synchronisation, capturable in
 * a graph. Low-res is fused (no intermediate image). Every descriptor is checked before the first
 * launch. src == dst is allowed for op 1 (in place) and op 0 (nothing is done), refused for ops 2, 3;
 * src and dst ranges that overlap without being equal are refused, and so is an output that overlaps
 * another image's input or output. */
int mx_corrupt_batch_u8(const mx_corrupt_desc* descs_host, int64_t n, const float* taps_host, int64_t ntaps_total,
                        const float* noise, mx_stream_t stream);
/* out[0], out[1] = rows, columns of the output tile one workgroup of mx_corrupt_batch_u8 owns. */
int mx_corrupt_batch_tile(int32_t out[2]);
/* Night, haze and rain for a whole batch in one launch (csrc/mx_weather.hip), each image with its own op,
 * parameters and size; the launch scheme of mx_corrupt_batch_u8 (one workgroup per output tile of one
 * image, descriptors as the kernel argument in chunks of 16 images: no workspace, no upload, no host
 * synchronisation, no allocation, capturable in a graph). The ops are this project's own definitions;
 * philox(counter x, y, z, w) below is Philox4x32-10 keyed (seed lo, seed hi), .x its first word.
 *   op 1 night (f32, every op rounded once): for byte i (flat index within the image) with value v,
 *     d = v * gain, s = sqrt(shot * d + read2), out = (u8)clip(d + s * g, 0, 255) (truncation), g =
 *     noise[i] when the call passes a field, else the Box-Muller normal of philox(i lo, i hi, 0x5eed, 0)
 *     that mx_corrupt_u8's noise uses.
 *   op 2 haze (integers, every product < 2^32): octaves o = 0..3 with cell c = 256 >> o, s = 8 - o;
 *     lattice L_o(j, i) = philox(i, j, 0x48415a45, o).x >> 16; for pixel (y, x): j = y >> s, i = x >> s,
 *     fy = y & (c-1), fx = x & (c-1), top = L(j,i)*(c-fx) + L(j,i+1)*fx, bot likewise from row j+1,
 *     v_o = (top*(c-fy) + bot*fy) >> 2s; S = sum (8 >> o) * v_o; S16 = (S * 4369) >> 16;
 *     alpha = lo + (((hi - lo) * S16) >> 16); per channel out = (v*(65536 - alpha) + air*alpha + 32768) >> 16.
 *   op 3 rain (integers): a drop head sits at (yy, xx) when, with X = xx + 4096 and
 *     w = philox(X >> 2, yy, 0x5241494e, 0), (w[X & 3] & 0xffff) < thr (components x, y, z, w);
 *     R = max over k in 0..len-1 of head(y + k, x + ((k*slant) >> 3)) * (256 - k*fade) (arithmetic shift);
 *     out = v + (((255 - v) * beta * R) >> 16). Streaks enter from outside the image through the same hash.
 * One descriptor per image, in a host array: */
typedef struct mx_weather_desc {
  const uint8_t* src; /* device, u8 [H][W][3] */
  uint8_t* dst;       /* device, u8 [H][W][3]; may be src (every op reads only the pixel it writes) */
  int32_t H, W;       /* 1..32768 each */
  int32_t op;         /* 1 night, 2 haze, 3 rain */
  float gain;         /* op 1: finite, >= 0 */
  uint64_t seed;      /* the Philox key of every op */
  float shot, read2;  /* op 1: finite, >= 0 */
  int32_t lo, hi, air; /* op 2: q16 0 <= lo <= hi <= 65535; air 0..255 */
  int32_t thr, len, slant, fade, beta; /* op 3: thr 0..65535, len 1..32, slant -8..8, fade >= 0 with
                                          (len-1)*fade < 256, beta 0..256 */
} mx_weather_desc;
/* noise: NULL, or one f32 field on the device for the whole call, laid out as in mx_corrupt_batch_u8 (the
 * images' [H][W][3] fields back to back in descriptor order, whatever their ops); only op 1 reads it.
 * Every descriptor is checked before the first launch and a failure returns MX_EINVAL: null pointers, a
 * bad op, a bad size, parameters out of range, src and dst ranges that overlap without being equal, an
 * output that overlaps another image's input or output. */
int mx_weather_batch_u8(const mx_weather_desc* descs_host, int64_t n, const float* noise, mx_stream_t stream);
/* out[0], out[1] = rows, columns of the output tile one workgroup of mx_weather_batch_u8 owns. */
int mx_weather_batch_tile(int32_t out[2]);

/* ---------------------------------------------------------------------------------------------
 * Detection overlays and side-by-side panels (csrc/mx_draw.hip): what scripts/demo_inference.py draws
 * with cv2 in the reference (draw_boxes, add_title, the resize + hstack of generate_comparison), on the
 * device, reading the fused tail's padded outputs (mx_det_select) where they lie. The text is the
 * project's own 5x7 bitmap font (csrc/mx_font5x7.h), not cv2's Hershey strokes, and the frames are not
 * anti-aliased, so the pixels are this project's definition, stated here exactly.
 * ------------------------------------------------------------------------------------------- */
/* One descriptor per image, in a host array: */
typedef struct mx_draw_desc {
  const uint8_t* src;    /* device, u8 [H][W][3] */
  uint8_t* dst;          /* device, u8 [bar + H][W][3]; may not overlap src */
  const float* boxes;    /* device, f32 [D][4] xyxy; may be NULL when D == 0 */
  const int64_t* labels; /* device, int64 [D]; may be NULL when D == 0 */
  const float* scores;   /* device, f32 [D], or NULL: ground-truth mode (no threshold, no score text) */
  const int32_t* count;  /* device, one int32: the rows 0..count-1 are candidates (count > D counts as D) */
  int32_t H, W;          /* 1..32768 each */
  int32_t D;             /* 0..2^20 */
  int32_t bar;           /* title-bar height, 0..1024; 0: none */
  int32_t title_len;     /* 0..64 */
  char title[64];        /* title bytes (no terminator needed) */
} mx_draw_desc;
/* One launch per chunk of 16 images, one workgroup per output tile (mx_draw_batch_tile) of one image;
 * descriptors, names and colours travel as the kernel argument: no workspace, no upload, no host
 * synchronisation, capturable in a graph. The result does not depend on the launch geometry.
 *   names_host: nnames <= 32 C strings of <= 15 bytes; entry k names label k + 1 (label 0 is the
 *     detector's background); an empty string, or a label outside 1..nnames, renders as "cls<label>"
 *     with the label in decimal ('-' for a negative one).
 *   colors_host: u8 [ncolors][3], ncolors <= 32; entry k colours label k + 1, the three bytes applied
 *     positionally to the image's channels 0, 1, 2 (the reference hands its RGB-looking triples to cv2
 *     on BGR images; a drop-in does the same). Any other label takes (200, 200, 200).
 *   label_scale, title_scale: integer font scales, 1..8. s = label_scale: th = 7*s and, for a text of
 *     L bytes, tw = 6*s*L.
 * Row i of an image is drawn when i < count and (scores == NULL or scores[i] >= conf_thr, false on NaN)
 * and its four coordinates are finite with |c| < 2^20; any other row draws nothing and is not counted.
 * (x1, y1, x2, y2) = the coordinates truncated toward zero. All ranges are inclusive, in image
 * coordinates, clipped to the image:
 *   frame: x1-1 <= x <= x2+1 and y1-1 <= y <= y2+1, less x1+1 <= x <= x2-1 and y1+1 <= y <= y2-1
 *          (thickness 2), in the class colour;
 *   plate: x1 <= x <= x1+tw+4 and y1-th-6 <= y <= y1, in the class colour;
 *   text:  white (255, 255, 255): font pixel (col, row) of character k covers the s x s block whose
 *          top-left is (x1 + 2 + 6*s*k + s*col, y1 - 3 - th + s*row). The text is the name, then in
 *          score mode one space and the score as mx_draw_format_score writes it.
 * Painter's order: within a row frame, plate, text; row i paints over every row j < i; a pixel no
 * primitive touches keeps the source value. Title bar: output rows 0..bar-1 are (40, 40, 40) with the
 * title in white at title_scale (tw, th from title_scale and title_len): glyph block top-left at
 * x = floor((W - tw) / 2), y = floor((bar + th) / 2) - th, clipped to the bar; the image occupies rows
 * bar..bar+H-1. drawn [n] int32 on the device: the number of rows drawn per image, or -1 when its
 * count < 0 (then nothing is drawn). Every byte of every output is written; n == 0 and D == 0 are
 * allowed. Every descriptor is checked before the first launch. */
int mx_draw_batch_u8(const mx_draw_desc* descs_host, int64_t n, const char* const* names_host, int32_t nnames,
                     const uint8_t* colors_host, int32_t ncolors, float conf_thr, int32_t label_scale,
                     int32_t title_scale, int32_t* drawn, mx_stream_t stream);
/* out[0], out[1] = rows, columns of the output tile one workgroup of mx_draw_batch_u8 owns; out[2] = the
 * capacity of its row list (an image with more candidate rows is binned in chunks of that many). */
int mx_draw_batch_tile(int32_t out[3]);
/* The glyph table: out [95][7] u8, ASCII 32..126, 7 row bytes each (top row first), bit 4 = the leftmost
 * of 5 columns. Host only. */
int mx_draw_font(uint8_t* out);
/* The score text of the overlay (host; the same function runs in the kernel): out = 4 bytes "d.dd" and
 * a terminating 0. n = rint((double)s * 100) (the product is exact; rint rounds half to even, so the
 * digits are those of printf("%.2f") of the exact f32 value), clamped to 0..999: s >= 9.995 prints
 * "9.99"; a negative s, -0 or NaN prints "0.00". */
int mx_draw_format_score(float s, char out[5]);
/* One panel of mx_panels_compose_u8: */
typedef struct mx_panel_desc {
  const uint8_t* src; /* device, u8 [h][w][3] */
  int32_t h, w;       /* 1..32768 each */
  int32_t dw;         /* the panel's width on the canvas, 1..32768 */
} mx_panel_desc;
/* One launch: canvas u8 [target_h][sum(dw_p) + 3*(P-1)][3], 1 <= P <= 8, 1 <= target_h <= 32768. Panel p
 * is resized to (dw_p, target_h) as cv2.resize's INTER_LINEAR does for u8 -- source index and the two
 * 11-bit fixed-point taps per axis from the pixel-centre mapping (d + 0.5) * (src / dst) - 0.5 rounded
 * to f32, clamped at the borders; horizontal pass, then the vertical combine
 * (((S0 >> 4) * b0) >> 16) + (((S1 >> 4) * b1) >> 16) + 2 >> 2 -- the taps of the corruption kernels'
 * low-res up-scale; a down-scale is plain bilinear with the same taps (no area averaging). Panels are
 * laid left to right, separated by 3 columns of (200, 200, 200). The canvas may not overlap a panel. */
int mx_panels_compose_u8(const mx_panel_desc* panels_host, int32_t P, int32_t target_h, uint8_t* canvas,
                         mx_stream_t stream);
/* Degradation statistics of a whole batch in one launch (csrc/mx_gate.hip), and a verdict per image from a
 * rule list over them: the blind gate in front of the restoration U-Net. The launch scheme of
 * mx_corrupt_batch_u8 (one workgroup per tile of one image, descriptors and rules as the kernel argument in
 * chunks of 16 images: no workspace, no upload, no host synchronisation, no allocation, capturable in a
 * graph); images of one call may differ in size. One memset of stats, then one launch per chunk.
 *   Luma Y = (77 R + 150 G + 29 B + 128) >> 8. The sums run over the interior pixels, rows 1..H-2 and
 *   columns 1..W-2 (no border rule), c the centre, Y(dy, dx) its neighbours, all exact int64:
 *     stats[b] = { N, IMM, DX2, DY2, DXX2, DYY2, G2, H2 }
 *     N    = (H-2)(W-2)
 *     IMM  = sum |Y(-1,-1) + Y(-1,1) + Y(1,-1) + Y(1,1) - 2 (Y(-1,0) + Y(1,0) + Y(0,-1) + Y(0,1)) + 4 c|
 *     DX2  = sum (Y(0,1) - Y(0,-1))^2            DY2  = sum (Y(1,0) - Y(-1,0))^2
 *     DXX2 = sum (Y(0,1) - 2 c + Y(0,-1))^2      DYY2 = sum (Y(1,0) - 2 c + Y(-1,0))^2
 *     G2   = DX2 + DY2                           H2   = DXX2 + DYY2
 *   |IMM term| <= 2040 and |DXX term| <= 510, so with H * W <= 2^24 every sum is below 2^47 and, with rule
 *   coefficients <= 65535, every product of a rule below 2^63.
 *   Rule r fires when a * stats[b][i] > b * stats[b][j]; the first rule that fires gives verdict[b], else
 *   default_verdict. 1 = restore, 0 = pass through. The verdict is evaluated on the device by the image's
 *   last-arriving workgroup (integer sums: independent of arrival order; a second call into the same
 *   buffers gives the same answer). */
typedef struct mx_gate_desc {
  const uint8_t* src; /* device, u8 [H][W][3] */
  int32_t H, W;       /* >= 3 each, H * W <= 2^24 */
  int32_t bgr;        /* 0: channel 0 is R; else channel 0 is B */
} mx_gate_desc;
typedef struct mx_gate_rule {
  int32_t i, j;    /* 0..7: the sums compared */
  int32_t a, b;    /* 0..65535 */
  int32_t verdict; /* 0 or 1 */
} mx_gate_rule;
/* stats: device int64 [n][8]; verdict: device int32 [n]. Refused before any launch (MX_EINVAL, with a
 * message): null pointers when n > 0, H < 3 or W < 3, H * W > 2^24, a rule out of bounds, nrules > 8, a
 * verdict that is not 0 or 1. n == 0 launches nothing. */
int mx_degradation_stats_u8(const mx_gate_desc* descs_host, int64_t n, const mx_gate_rule* rules_host, int32_t nrules,
                            int32_t default_verdict, int64_t* stats, int32_t* verdict, mx_stream_t stream);
/* out[0], out[1] = rows, columns of the tile of interior pixels one workgroup of mx_degradation_stats_u8 owns. */
int mx_degradation_stats_tile(int32_t out[2]);
/* Blind non-local means over a whole batch in one launch (csrc/mx_denoise.hip): the pixel branch for the
 * images the gate's noise rule recognises, with the strength taken per image from the gate's own sums on the
 * device. The launch scheme of mx_degradation_stats_u8 (one workgroup per output tile of one image, descriptors
 * as the kernel argument in chunks of 16 images: no workspace, no upload, no host synchronisation, no
 * allocation, capturable in a graph); images of one call may differ in size. Every value is an unsigned integer.
 *   Constants: patch radius 2 (5 x 5), search radius 5 (11 x 11 = 121 candidates, the centre included);
 *   coordinates outside the image clamp to the nearest pixel; luma Y = (77 R + 150 G + 29 B + 128) >> 8 (bgr
 *   as in mx_gate_desc); LUT[i] = round(4096 * exp(-i / 16)) for i = 0..127 as committed literals
 *   (mx_denoise_nlm_lut), weight 0 from index 128 up.
 *   Per image: s8 = the luma noise sigma in 1 / 256 grey levels.
 *     sigma_q8 in 1..65535: s8 = sigma_q8 and the image is denoised.
 *     sigma_q8 == 0 (blind): from stats[b] = { N, IMM, ... } as mx_degradation_stats_u8 wrote them,
 *       a = (IMM << 8) / N, s8 = (a * 13689) >> 16 (13689 / 65536 = 1.2533 / 6, Immerkaer's scale); the image
 *       is denoised only when rule_a * IMM > rule_b * N (the gate's noise rule: 10, 383).
 *     With a verdict array, an image is denoised only if verdict[b] == 0 as well (the U-Net's images are left
 *     alone).
 *     T0 = (50 * s8 * s8) >> 16      (the expected patch distance of pure noise, 25 * 2 sigma^2)
 *     D  = max((25 * k16 * k16 * s8 * s8) >> 24, 1)      (h = k16 / 16 sigma; k16 = 6: h = 0.375 sigma)
 *     Q  = (1 << 24) / D
 *     An image that is not denoised has dst = the bytes of src. applied[b] = 1 for a denoised image, else 0.
 *   Per pixel p and candidate q = p + (dy, dx), |dy|, |dx| <= 5:
 *     d   = sum over |u|, |v| <= 2 of (Y(p + uv) - Y(q + uv))^2        (< 2^21)
 *     t   = max(d - T0, 0)
 *     idx = min((t * Q) >> 20, 128)                                     (t * Q < 2^45, in 64 bits)
 *     w   = LUT[idx], Wsum = sum w  (>= 4096: the centre has t = 0; < 2^19)
 *     out_c(p) = (sum w * X_c(q) + (Wsum >> 1)) / Wsum per channel      (sum w * X < 2^27)
 *   X is read from src: results never feed back. With valid stats a <= 2040 * 256 and s8 < 2^17, so every
 *   product above stays below 2^63. */
typedef struct mx_nlm_desc {
  const uint8_t* src; /* device, u8 [H][W][3] */
  uint8_t* dst;       /* device, u8 [H][W][3]; may overlap no src of the call */
  int32_t H, W;       /* >= 1 each (>= 3 for a blind image), H * W <= 2^24 */
  int32_t bgr;        /* 0: channel 0 is R; else channel 0 is B */
  int32_t sigma_q8;   /* 0: blind, from stats; 1..65535: the luma sigma in 1 / 256 grey levels */
} mx_nlm_desc;
/* stats: device int64 [n][8], may be NULL when every sigma_q8 > 0; verdict: device int32 [n] or NULL; applied:
 * device int32 [n] or NULL. Refused before any launch (MX_EINVAL, with a message): null pointers, H or W < 1,
 * H * W > 2^24, sigma_q8 outside 0..65535, a blind image without stats or with H or W < 3, k16 outside 1..64,
 * rule coefficients outside 0..65535, a dst that overlaps a src (a tile reads pixels another tile writes).
 * n == 0 launches nothing. */
int mx_denoise_nlm_u8(const mx_nlm_desc* descs_host, int64_t n, const int64_t* stats, const int32_t* verdict,
                      int32_t rule_a, int32_t rule_b, int32_t k16, int32_t* applied, mx_stream_t stream);
/* out[0], out[1] = rows, columns of the output tile one workgroup of mx_denoise_nlm_u8 owns. */
int mx_denoise_nlm_tile(int32_t out[2]);
/* The 128 weights of mx_denoise_nlm_u8's table. Host only. */
int mx_denoise_nlm_lut(int32_t out[128]);
/* GeneralizedRCNNTransform (normalize, zero-pad to /32) fused with ToDtype(scale=True):
 * u8 HWC [B,H,W,3] -> NHWC [B, Hp, Wp, Cp] dtype, (x/255 - mean)/std, zero padding; Cp >= 3 (extra
 * channels zero, for the conv stem's 8-channel gather). */
int mx_normalize_pad(const uint8_t* img, int64_t B, int64_t H, int64_t W, const float* mean3_host,
                     const float* std3_host, int64_t Hp, int64_t Wp, int64_t Cp, int dtype, void* out,
                     mx_stream_t stream);

/* GeneralizedRCNNTransform for images that need a resize (torchvision 0.20.1 transform.py
 * _resize_image_and_masks -> F.interpolate(scale_factor, bilinear, align_corners=False,
 * recompute_scale_factor=True), reached via the model call at train_frcnn_baseline.py:171 and
 * eval_all.py:111 on VisDrone frames of any size), fused with ToDtype(scale=True), normalize and
 * batch_images' zero padding: B u8 HWC images imgs[b] [Hs[b], Ws[b], 3] (device pointers; sizes host
 * arrays) -> NHWC [B, Hp, Wp, Cp] dtype; image b fills its [nhs[b], nws[b]] corner (nh = floor(H*s),
 * computed by the caller as torch does), the rest is zero. Bilinear weights as torch's CUDA kernel:
 * scale = (float)H / nh, src = scale * (dst + 0.5) - 0.5 (clamped at 0). */
int mx_resize_normalize_pad(const uint8_t* const* imgs, const int64_t* Hs, const int64_t* Ws, const int64_t* nhs,
                            const int64_t* nws, int64_t B, const float* mean3_host, const float* std3_host,
                            int64_t Hp, int64_t Wp, int64_t Cp, int dtype, void* out, mx_stream_t stream);
/* RPN head outputs -> torchvision's concatenated (objectness [N, Atot], pred_deltas [N, Atot, 4]) in
 * one pass (concat_box_prediction_layers, rpn.py; the reference model's RPN via train_frcnn_baseline.py:171)
 * and the reverse for the backward. o0: level 0's [N, H0, W0, 5A] head output (A logits then A x 4
 * deltas per pixel); ocv: the [N, Hc, Wc, 5A] canvas holding levels 1..ncv at rects[l] = (y, x, h, w).
 * merge writes every element of g0 / gcv (frame pixels 0; gobj / gdel nullable = zero). */
int mx_rpn_head_split(const float* o0, int64_t H0, int64_t W0, const float* ocv, int64_t Hc, int64_t Wc,
                      const int32_t* rects, int ncv, int64_t N, int A, float* obj, float* del, mx_stream_t stream);
int mx_rpn_head_merge(const float* gobj, const float* gdel, int64_t H0, int64_t W0, int64_t Hc, int64_t Wc,
                      const int32_t* rects, int ncv, int64_t N, int A, float* g0, float* gcv, mx_stream_t stream);
/* Zero-framed canvas of n NHWC maps (frcnn.RPNHead: the small FPN levels as one conv input):
 * pack writes every element of cv [N, Hc, Wc, C] (map l at rects[l] = (y, x, h, w), 0 elsewhere);
 * unpack is its backward: grads[l] = the slice of gcv (+ add[l], nullable list / entries). C % 8 == 0;
 * dtype MX_F32 / MX_BF16 for every buffer. */
int mx_canvas_pack(const void* const* maps, const int32_t* rects, int n, int64_t N, int64_t Hc, int64_t Wc, int64_t C,
                   int dtype, void* cv, mx_stream_t stream);
int mx_canvas_unpack(const void* gcv, const int32_t* rects, int n, int64_t N, int64_t Hc, int64_t Wc, int64_t C,
                     int dtype, const void* const* add, void* const* grads, mx_stream_t stream);
/* The same for the reference loader's own image tensors: ToDtype(float32, scale=True) output, f32 CHW
 * [3, Hs[b], Ws[b]] contiguous (train_frcnn_baseline.py:50-54 build_transforms, fed to the model at :171).
 * A float image equal to u8 * (float)(1/255) gives the bit-identical batch of mx_resize_normalize_pad;
 * no resize (nh = H, nw = W) reproduces normalize + pad exactly. */
int mx_resize_normalize_pad_f32(const float* const* imgs_chw, const int64_t* Hs, const int64_t* Ws, const int64_t* nhs,
                                const int64_t* nws, int64_t B, const float* mean3_host, const float* std3_host,
                                int64_t Hp, int64_t Wp, int64_t Cp, int dtype, void* out, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Convolution (implicit GEMM on MFMA, bf16 in / f32 accumulate), NHWC x KRSC.
 * Replaces the cuDNN convs of ResNet-50 / FPN / RPN head / box head (torchvision model reached at
 * train_frcnn_baseline.py:171) and the U-Net convs (restoration_net.py:17-30, restore_testsets.py:68).
 *   fwd:   y[N,Ho,Wo,K] = conv(x[N,H,W,C], w[K,R,S,C]) (+bias[K] f32, nullable), output dtype
 *          ydtype; stats (nullable) receives per-block column partial sums for train-mode
 *          BatchNorm: stats[2][mblocks][K] f32 (sum, sum of squares) of the f32 accumulators.
 *   dgrad: dx[N,H,W,C] = conv_transpose(dy[N,Ho,Wo,K], w)   (bf16; strides 1 and 2)
 *   wgrad: dw[K,R,S,C] f32 = sum over N,Ho,Wo dy (x) x      (overwritten; the pixel axis is split
 *          into per-split partials in a workspace and summed by a reduce kernel — no atomics)
 *   C % 8 == 0 is required (the stem input is padded to 8 channels).
 *   stride_h / stride_w, pad_h / pad_w and R / S are independent (asymmetric strides, pads and
 *   filters are supported by every pass); an output map may be smaller than the filter.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t N, H, W, C, K, R, S, Ho, Wo;
  int32_t stride_h, stride_w, pad_h, pad_w;
} mx_conv_shape;
/* Launch settings of ONE call: the six values the per-shape tuner varies. The entries that take a
 * `const mx_conv_cfg* cfg` (last parameter) read it as follows: NULL = the process defaults (the
 * mx_conv_set_* values below); otherwise the cfg replaces all six values for that call only and no
 * process default is read or written for them. A workspace query and the launch that consumes its
 * workspace must be given the same cfg. A cfg outside the setters' ranges (or reserved != 0) is
 * MX_EINVAL before any HIP call (workspace queries: 0). The convenience forms without a cfg
 * parameter use the process defaults. */
typedef struct mx_conv_cfg {
  int32_t tile_rows, tile_cols; /* mx_conv_set_tile       (0,0 = automatic) */
  int32_t max_splits;           /* mx_conv_set_max_splits (0 = automatic)   */
  int32_t stages;               /* mx_conv_set_stages     (0 = automatic)   */
  int32_t wgrad_variant;        /* mx_conv_set_wgrad_variant                */
  int32_t reserved;             /* must be 0 */
  int64_t wgrad_target;         /* mx_conv_set_wgrad_target (0 = automatic) */
} mx_conv_cfg;
int64_t mx_conv_mblocks(const mx_conv_shape* s);
int mx_conv2d_fwd(const mx_conv_shape* s, const uint16_t* x, const uint16_t* w, const float* bias, void* y,
                  int ydtype, float* stats, mx_stream_t stream);
int mx_conv2d_dgrad(const mx_conv_shape* s, const uint16_t* dy, const uint16_t* w, uint16_t* dx,
                    mx_stream_t stream);
/* Hot-path forms. fwd_ex adds a fused epilogue: + residual[M][K] (bf16, nullable), then activation
 * (0 none, 1 ReLU, 2 LeakyReLU(0.2)) — the eval-mode conv+folded-BN(+add)+act of the backbone and
 * the U-Net. dgrad_t takes the weight in the dgrad layout written by mx_conv_pack_weight (the
 * plain mx_conv2d_fwd / mx_conv2d_dgrad allocate their temporaries with hipMallocAsync; the _ex / _t
 * forms take caller workspaces and are the graph-capturable hot path). Small grids split K: their
 * f32 partials go to `ws` (mx_conv_workspace bytes) and a reduce kernel applies the epilogue.
 * dgrad runs one dense GEMM per stride-parity class of dx (strides 1 and 2): rows with
 * h % st == ph only receive taps r == (ph + pad) % st, so no MFMA work is spent on the zero taps
 * of a strided conv. */
int mx_conv2d_fwd_ex(const mx_conv_shape* s, const uint16_t* x, const uint16_t* w, const float* bias,
                     const uint16_t* residual, int act, void* y, int ydtype, float* stats, void* ws, size_t ws_bytes,
                     mx_stream_t stream, const mx_conv_cfg* cfg);
/* Split workspace for pass 0 (fwd) / 1 (dgrad) / 2 (wgrad): 0 when the grid fills the chip unsplit. */
size_t mx_conv_workspace(const mx_conv_shape* s, int pass, const mx_conv_cfg* cfg);
/* Process defaults of the launch settings, for tools and A/B tests: what a call with cfg == NULL
 * uses. variant, loader and korder are whole-process diagnostics with no per-call form; the others
 * are the fields of mx_conv_cfg, and a call with a cfg neither reads nor changes them (a tuned launch
 * does not reset them). fwd/dgrad variant: 0 register-staged, 1/2 direct-to-LDS 2-stage, 3..6
 * multi-stage direct-to-LDS (BK32x3, BK64x2, BK32x4, BK64x3), 7 (default) per-launch choice between
 * 3 and 4. wgrad variant: 0 32-pixel K-tiles, 1 64-pixel, 2 direct-to-LDS, 3 (default) buffer
 * descriptors, 4 / 5 the bf16x3 128x256 / 256x256 blocks (bf16: as 3). */
int mx_conv_set_variant(int variant);
int mx_conv_get_variant(void);
int mx_conv_set_wgrad_variant(int variant);
int mx_conv_get_wgrad_variant(void);
/* Per-step weight preparation from the f32 master parameter w[Kout][Cin][R][S] (torch layout) in
 * one pass (split != 0: every layout as hi / lo bf16 planes, see mx_pack_desc.flags bit 1): wk = [Kout][R][S][s->C] bf16 (input channels zero-padded to s->C; nullable) and
 * wt = the dgrad operand (nullable): for each tap-parity class (r0, s0) = (r % st_h, s % st_w), in
 * order r0*st_w + s0, a contiguous block [s->C][Rc][Sc][s->K] (output channels zero-padded to s->K);
 * for stride 1 this is the plain [C][R][S][K] transpose. Uses s->C, K, R, S, strides, pads.
 * Replaces the per-step .to(bfloat16) weight casts of the reference's autocast-free fp32 model. */
int mx_conv_pack_weight(const mx_conv_shape* s, const float* w, int64_t Cin, int64_t Kout, uint16_t* wk, uint16_t* wt,
                        int split, mx_stream_t stream);
size_t mx_conv_dgrad_weight_elems(const mx_conv_shape* s, int64_t Cpad, int64_t Kpad);
/* The same packing for a list of weights in ONE launch (per-step operand preparation of a whole
 * model). A job: f32 w[Kout][Cin][R][S] -> wk [Kout][R][S][Cpad] (nullable) and wt, the dgrad layout
 * with Cpad / Kpad (nullable). `plan` is a caller-owned device buffer of mx_conv_pack_plan_bytes(njobs)
 * holding the job table; upload=1 (re)writes it from `jobs` (synchronizes the stream; do it when the
 * job list changes), upload=0 reuses it. */
typedef struct {
  const float* w;
  uint16_t* wk;
  uint16_t* wt;
  int64_t Cin, Kout, Cpad, Kpad;
  int32_t R, S, stride_h, stride_w, pad_h, pad_w;
  int32_t flags; /* bit 0: "dense" dgrad layout [R][S][Cpad][Kpad] for a conv whose output is 1x1 (FC6 as a
                    valid 7x7 conv): its dgrad runs as the 1x1 GEMM dX[N, R*S*C] = dY[N, K] * W;
                    bit 1: split -- each layout written as two bf16 planes, hi = bf16(w) then
                    lo = bf16(w - hi) (the bf16x3 operands of the *_x3 convolutions; buffers twice
                    the size) */
} mx_pack_desc;
size_t mx_conv_pack_plan_bytes(int64_t njobs);
int mx_conv_pack_batched(const mx_pack_desc* jobs, int64_t njobs, void* plan, size_t plan_bytes, int upload,
                         mx_stream_t stream);
/* SGD step (torch.optim.SGD semantics, see mx_sgd_step) fused with the per-step conv operand pack:
 * a parameter with `pack` >= 0 is the f32 weight packs[pack].w, and its update and its wk / wt layouts
 * (exactly what mx_sgd_step followed by mx_conv_pack_batched would write) come out of one pass; the
 * others take plain multi-tensor SGD blocks of the same launch (scripts/train_frcnn_baseline.py:149-153,
 * 174-176: optimizer.step() then the next forward's weights). Fused packs take R*S <= 49.
 * mx_sgd_pack_build fills a HOST buffer of mx_sgd_pack_plan_bytes(nparams) (no device calls) and
 * returns the grid size and dynamic LDS bytes; the caller copies it to device memory (stream-ordered)
 * and launches mx_sgd_pack_step with it and a device array of the nparams gradient pointers. */
typedef struct {
  float* p;
  float* buf;    /* momentum buffer */
  int64_t n;
  int32_t first; /* 1: the buffer starts from this step's d (torch's first momentum step) */
  int32_t pack;  /* index into packs[] or -1 */
} mx_sgd_param;
size_t mx_sgd_pack_plan_bytes(int64_t nparams);
int mx_sgd_pack_build(const mx_sgd_param* params, int64_t nparams, const mx_pack_desc* packs, void* host_plan,
                      size_t plan_bytes, int64_t* blocks, size_t* lds_bytes);
int mx_sgd_pack_step(const void* plan, const float* const* grads, int64_t nparams, int64_t blocks, size_t lds_bytes,
                     float lr, float momentum, float dampening, float weight_decay, int nesterov, mx_stream_t stream);
/* AdamW step (torch.optim.AdamW semantics, see mx_adamw_step) fused with the per-step conv operand
 * pack, for the restoration U-Net's loop (train_restoration.py:246 builds AdamW(lr 1e-3, weight_decay
 * 1e-4), :272 steps it, and the next forward packs the new weights): a parameter with `pack` >= 0 is the
 * f32 weight packs[pack].w, and its update and its wk / wt layouts (exactly what mx_adamw_step followed
 * by mx_conv_pack_batched would write: split hi / lo planes, the stride-parity dgrad layout, the dense
 * flag, zero-padded channels) come out of one pass; the others take plain multi-tensor AdamW blocks
 * of the same launch. Fused packs take R*S <= 49. One launch serves a whole parameter group that
 * shares one step number (`step`: the number after this step, >= 1); the hyper-parameters are launch
 * arguments, so a schedule that changes lr needs no new plan.
 * mx_adamw_pack_build fills a HOST buffer of mx_adamw_pack_plan_bytes(nparams) (no device calls; the
 * conventions and tiles of mx_sgd_pack_build) and returns the grid size and dynamic LDS bytes; the
 * caller copies it to device memory (stream-ordered) and launches mx_adamw_pack_step with it and a
 * device array of the nparams gradient pointers. */
typedef struct {
  float* p;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;
  int32_t pack;     /* index into packs[] or -1 */
  int32_t reserved; /* 0 */
} mx_adamw_param;
size_t mx_adamw_pack_plan_bytes(int64_t nparams);
int mx_adamw_pack_build(const mx_adamw_param* params, int64_t nparams, const mx_pack_desc* packs, void* host_plan,
                        size_t plan_bytes, int64_t* blocks, size_t* lds_bytes);
int mx_adamw_pack_step(const void* plan, const float* const* grads, int64_t nparams, int64_t blocks, size_t lds_bytes,
                       int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                       mx_stream_t stream);
/* [K][RS][C] -> [C][RS][K] bf16 (the stride-1 dgrad layout). */
int mx_conv_transpose_weight(const uint16_t* w, int64_t K, int64_t RS, int64_t C, uint16_t* wt, mx_stream_t stream);
int mx_conv2d_dgrad_t(const mx_conv_shape* s, const uint16_t* dy, const uint16_t* wt, uint16_t* dx, void* ws,
                      size_t ws_bytes, mx_stream_t stream);
/* mx_conv2d_dgrad_t plus a bf16 [N][H][W][C] tensor added to dx in the epilogue before the single
 * bf16 rounding (strides 1 and 2: each parity class adds it at the pixels it writes): the gradient of
 * an input that also feeds another branch (ResNet bottleneck x -> conv1 and x -> + identity, a stage
 * output read by the next stage and the FPN) without a separate add pass. */
int mx_conv2d_dgrad_ex(const mx_conv_shape* s, const uint16_t* dy, const uint16_t* wt, const uint16_t* residual,
                       uint16_t* dx, void* ws, size_t ws_bytes, mx_stream_t stream, const mx_conv_cfg* cfg);
/* mx_conv2d_dgrad_ex whose output dx is the incoming gradient of a train-mode BatchNorm (+act)
 * that produced z -> y with batch mean / invstd: the epilogue also writes, per 64-row block, the
 * column sums of g = bf16(dx) * act'(y) and g * (z - mean) * invstd into part [2][part_mb][C]
 * (part_mb = cdiv(N*H*W, 64)); mx_bn_bwd_finalize then replaces mx_bn_bwd_reduce_ex (no second
 * pass over dx, y, z). Stride 1. */
int mx_conv2d_dgrad_bnb(const mx_conv_shape* s, const uint16_t* dy, const uint16_t* wt, const uint16_t* residual,
                        uint16_t* dx, const uint16_t* y, const uint16_t* z, const float* mean, const float* invstd,
                        int act, float* part, int64_t part_mb, void* ws, size_t ws_bytes, mx_stream_t stream,
                        const mx_conv_cfg* cfg);
int mx_conv2d_wgrad(const mx_conv_shape* s, const uint16_t* dy, const uint16_t* x, float* dw, mx_stream_t stream);
/* Hot-path wgrad: dw written directly in layout 0 ([Kout][R][S][Cin]) or 1 ([Kout][Cin][R][S], the
 * torch parameter layout, so the result is the weight's .grad as is), dropping the zero-padded
 * channels (Kout <= s->K, Cin <= s->C); ws = mx_conv_workspace(s, 2) bytes. */
int mx_conv2d_wgrad_ex(const mx_conv_shape* s, const uint16_t* dy, const uint16_t* x, float* dw, int64_t Kout,
                       int64_t Cin, int layout, void* ws, size_t ws_bytes, mx_stream_t stream, const mx_conv_cfg* cfg);
/* fwd/dgrad operand loader knob: 1 (default) buffer descriptors with wave-uniform tap offsets where
 * the shape allows (input channels % 32 == 0, R*S <= 64, operands < 2 GiB), 0 per-lane global loads. */
int mx_conv_set_loader(int loader);
/* fwd/dgrad block-tile override for tuning: (0, 0) automatic, else rows 64/128/256 x columns 64/128/256
 * (256 rows: the bf16x3 kernels only, as 256 x 128 tiles; the bf16 kernels run 128 rows instead). */
int mx_conv_set_tile(int block_rows, int block_cols);
/* Upper bound on the split-K factor of fwd / dgrad launches (0 = automatic; tuning only). */
int mx_conv_set_max_splits(int max_splits);
/* LDS ring depth of the 64x128 / 128x128 buffer-descriptor kernels (0 = automatic; tuning only). */
int mx_conv_set_stages(int stages);
/* K-tile order of the buffer-descriptor conv kernels: 0 tap-major, 1 (default) channel-major (all taps
   of a 32-channel chunk before the next chunk: cross-tap re-reads of the gathered rows hit L2). */
int mx_conv_set_korder(int order);
/* wgrad grid sizing: the pixel axis is split until ~blocks workgroups (0 = one wave of resident blocks). */
int mx_conv_set_wgrad_target(int64_t blocks);
/* The calling thread's last conv launch (fwd / dgrad / wgrad, bf16 and bf16x3 entries), for tests that
 * assert which path a shape took: out[0] pass (0 fwd, 1 dgrad, 2 wgrad), out[1] x out[2] block tile
 * (rows x columns), out[3] K splits (wgrad: pixel splits) launched, out[4] output tiles, out[5] 1 when
 * a buffer-descriptor kernel ran, out[6] kernel kind (bf16 fwd/dgrad: the mx_conv_set_variant number
 * launched; bf16 wgrad: the mx_conv_set_wgrad_variant number launched, 0 when the buffer kernel's map
 * guard fell back to the register kernel; bf16x3 fwd/dgrad: 100 + the mx_conv_set_stages alternative;
 * bf16x3 wgrad: 103 / 104 / 105 for the 128x128 / 128x256 / 256x256 block, 106 for the tile-list
 * 128x128 wgrad (mx_conv2d_wgrad_x3_rows); 107 for the rows dgrad (mx_conv2d_dgrad_x3_rows), whose out[3]
 * is 1 and out[4] the blocks launched for the list's capacity), out[7] launches the entry
 * has issued (stride-2 dgrad: the non-empty parity classes; the record is that of the last one).
 * MX_EINVAL before the thread's first launch. */
int mx_conv_last_launch(int32_t out[8]);

/* ---------------------------------------------------------------------------------------------
 * Precision-faithful convolution (bf16x3): the reference trains and evaluates its convs in fp32
 * (TF32 on Ampere; train_frcnn_baseline.py:139-176, no autocast; U-Net restore_testsets.py:64-68).
 * Activations, gradients and outputs are f32 NHWC; every product is computed as
 * hi*hi + hi*lo + lo*hi of the operands' bf16 hi/lo split (three v_mfma_f32_16x16x32_bf16 per
 * K-step, f32 accumulation; ~2^-16 relative per product against TF32's 2^-11). Weights are the
 * split planes written by mx_conv_pack_weight / mx_conv_pack_batched with split set: w [2][K][R][S][C]
 * (fwd), wt [2][dgrad layout] (dgrad). Same shapes, epilogues, BN statistics, split-K workspaces
 * (mx_conv_workspace_x3) and layouts as the bf16 entries above.
 *   dgrad_x3: part != NULL adds the mx_conv2d_dgrad_bnb BN-backward partials (y, z, mean, invstd, act
 *   of the BN whose output gradient dx is; stride 1), else those arguments are ignored.
 * ------------------------------------------------------------------------------------------- */
size_t mx_conv_workspace_x3(const mx_conv_shape* s, int pass, const mx_conv_cfg* cfg);
int mx_conv2d_fwd_x3(const mx_conv_shape* s, const float* x, const uint16_t* w, const float* bias, const float* residual,
                     int act, float* y, float* stats, void* ws, size_t ws_bytes, mx_stream_t stream,
                     const mx_conv_cfg* cfg);
/* The ResNet stem as mx_conv2d_fwd_x3 (torchvision resnet50 conv1, reached from
 * train_frcnn_baseline.py:171 through the detector's backbone): R = S = 7, K = 64, the same packed w
 * [2][64][7][7][C] and outputs (y = act(conv + bias), optional BN statistics partials, no residual),
 * with only channels 0..3 of x and w read -- the caller's real input channels are <= 4 (RGB padded
 * to C = 8 with zeros). One MFMA K-step per filter row: 224 products per output instead of 416. */
int mx_conv2d_stem_x3(const mx_conv_shape* s, const float* x, const uint16_t* w, const float* bias, int act, float* y,
                      float* stats, mx_stream_t stream);
int mx_conv2d_dgrad_x3(const mx_conv_shape* s, const float* dy, const uint16_t* wt, const float* residual, float* dx,
                       const float* y, const float* z, const float* mean, const float* invstd, int act, float* part,
                       int64_t part_mb, void* ws, size_t ws_bytes, mx_stream_t stream, const mx_conv_cfg* cfg);
int mx_conv2d_wgrad_x3(const mx_conv_shape* s, const float* dy, const float* x, float* dw, int64_t Kout, int64_t Cin,
                       int layout, void* ws, size_t ws_bytes, mx_stream_t stream, const mx_conv_cfg* cfg);

/* Row-sparse backward of the RPN head (Faster R-CNN training: the RPN loss gives a gradient to at
 * most B = batch_size_per_image sampled anchors per image, every other element of the raw head maps'
 * gradient is an exact zero).
 * mx_rpn_rows_build: from the gradient g of a raw head map [N][H][W][C] f32, the ascending lists of
 * flat pixel indices (n*H + h)*W + w of S0 = pixels with any nonzero bit pattern among their C values
 * (the sign bit ignored: -0.0 does not mark), S1 = S0 dilated by the 3x3 neighbourhood clipped to
 * the pixel's own image, S2 = S1 dilated again; `levels` (1..3) of them are built into rows0..2 of
 * capacities cap0..2 (<= N*H*W; mx_rpn_rows_capacity(P, N*B, level) = min(P, N*B * {1, 9, 25})).
 * counts[l] = the true number of pixels of list l; a list longer than its capacity is cut there
 * (nothing is written past it) and *flag is set to 1 (sticky: never cleared by the library).
 * ws: mx_rpn_rows_workspace(N*H*W) bytes. No atomics, no sort: a bitmap per list and an ordered
 * popcount scan, so the result is deterministic.
 * mx_rpn_tiles_build: the same three sets as ascending lists of the 32-pixel K-steps that hold one of
 * their pixels (index p / 32 over the flat pixels: the aligned groups the x3 wgrad kernel multiplies
 * per MFMA step), capacities mx_rpn_tiles_capacity(P, N*B, level) = min(ceil(P / 32), N*B * {1, 6, 10});
 * counts, overflow, flag and workspace as above.
 * mx_conv2d_wgrad_x3_rows: mx_conv2d_wgrad_x3 (128 x 128 kernel: cfg NULL or wgrad_variant 3; others
 * are refused) with the same cfg, geometry, workspace (mx_conv_workspace_x3 pass 2) and split
 * partials, each block running only those K-steps of its split that tiles / ntiles list
 * (min(*ntiles, cap) entries of an mx_rpn_tiles_build list are read). dy stays the dense-addressed
 * [N][Ho][Wo][K] map and must be zero in every K-step not listed: a skipped step would have added
 * exact zeros to every accumulator, so for finite operands dw equals mx_conv2d_wgrad_x3's bit for bit. */
int64_t mx_rpn_rows_capacity(int64_t P, int64_t NB, int level);
size_t mx_rpn_rows_workspace(int64_t P);
int mx_rpn_rows_build(const float* g, int64_t N, int64_t H, int64_t W, int64_t C, int levels, int32_t* rows0,
                      int64_t cap0, int32_t* rows1, int64_t cap1, int32_t* rows2, int64_t cap2, int32_t* counts,
                      int32_t* flag, void* ws, size_t ws_bytes, mx_stream_t stream);
int64_t mx_rpn_tiles_capacity(int64_t P, int64_t NB, int level);
int mx_rpn_tiles_build(const float* g, int64_t N, int64_t H, int64_t W, int64_t C, int levels, int32_t* tiles0,
                       int64_t cap0, int32_t* tiles1, int64_t cap1, int32_t* tiles2, int64_t cap2, int32_t* counts,
                       int32_t* flag, void* ws, size_t ws_bytes, mx_stream_t stream);
int mx_conv2d_wgrad_x3_rows(const mx_conv_shape* s, const float* dy, const float* x, float* dw, int64_t Kout,
                            int64_t Cin, int layout, const int32_t* tiles, const int32_t* ntiles, int64_t cap, void* ws,
                            size_t ws_bytes, mx_stream_t stream, const mx_conv_cfg* cfg);
/* mx_rpn_lists_build: what one backward step of a head map needs, from one mark and two dilations: the
 * pixel lists S0, S1, S2 of mx_rpn_rows_build (rows0..2, counts[3]) and the K-step lists S0, S1 of
 * mx_rpn_tiles_build (tiles0..1, tcounts[2]), each compacted from the same bitmap; capacities, cut
 * lists, flag and workspace as for the two entries above.
 * mx_conv2d_dgrad_x3_rows: the stride-1 mx_conv2d_dgrad_x3 on listed pixels only. rows: ascending flat
 * pixel indices into [N][H][W] (min(*nrows, cap) entries are read; the grid is sized by cap, blocks
 * past the count exit at once); for each listed pixel p, dx[p] = dgrad(dy)[p] (+ residual[p]) -- the
 * same kernel instance, K order and sum as the dense launch of this shape and cfg, so the same bits;
 * every other row of dx is left untouched (dx may be the residual buffer: an in-place add). An entry
 * outside [0, N*H*W) is an invalid row: nothing is read or stored for it. dy is the dense-addressed
 * map and must be zero wherever the dense gradient is. MX_EUNSUPPORTED, before any launch, when the
 * dense launch of the shape and cfg is not an unsplit wide-wave 128- or 64-row x 128-column tile of
 * the buffer kernel (mx_conv2d_dgrad_x3_rows_supported: 1 when it is): the caller runs the dense entry.
 * mx_act_bias_bwd_rows: mx_act_bias_bwd (act 1, f32 in and out, K % 8 == 0) on listed rows only, on the
 * dense launch's grid and row partition: g[r] = (gy[r] * mask[r % mask_period]) * act'(y[r]) for the
 * listed rows r (mask nullable: no factor), other rows of g are not written; db (nullable) and the
 * workspace as mx_act_bias_bwd. gy zero off the list: g's listed rows and db are the dense values. */
int mx_rpn_lists_build(const float* g, int64_t N, int64_t H, int64_t W, int64_t C, int32_t* rows0, int64_t cap0,
                       int32_t* rows1, int64_t cap1, int32_t* rows2, int64_t cap2, int32_t* counts, int32_t* tiles0,
                       int64_t tcap0, int32_t* tiles1, int64_t tcap1, int32_t* tcounts, int32_t* flag, void* ws,
                       size_t ws_bytes, mx_stream_t stream);
int mx_conv2d_dgrad_x3_rows_supported(const mx_conv_shape* s, const mx_conv_cfg* cfg);
int mx_conv2d_dgrad_x3_rows(const mx_conv_shape* s, const float* dy, const uint16_t* wt, const float* residual, float* dx,
                            const int32_t* rows, const int32_t* nrows, int64_t cap, mx_stream_t stream,
                            const mx_conv_cfg* cfg);
int mx_act_bias_bwd_rows(const float* gy, const float* y, const float* mask, int64_t mask_period, int64_t M, int64_t K,
                         const int32_t* rows, const int32_t* nrows, int64_t cap, float* g, float* db, void* ws,
                         size_t ws_bytes, mx_stream_t stream);

/* NHWC pooling / resampling (dtype MX_BF16 or MX_F32 storage, C % 8 == 0).
 * maxpool: F.max_pool2d (ResNet stem k3 s2 p1 — torchvision resnet50 reached at
 *   train_frcnn_baseline.py:139; U-Net MaxPool2d(2), restoration_net.py:39); argmax (nullable,
 *   int32 [N,Ho,Wo,C]) feeds the gather-form backward.
 * upsample_nearest: F.interpolate(mode="nearest", size=(Ho,Wo)) of the FPN top-down path, fused with
 *   the lateral add (y = up(x) + add, add nullable); backward sums each source's destinations. */
int mx_maxpool_fwd(const void* x, int dtype, int64_t N, int64_t H, int64_t W, int64_t C, int k, int stride, int pad,
                   void* y, int32_t* argmax, mx_stream_t stream);
int mx_maxpool_bwd(const void* gy, int dtype, const int32_t* argmax, int64_t N, int64_t H, int64_t W, int64_t C, int k,
                   int stride, int pad, void* gx, mx_stream_t stream);
int mx_upsample_nearest_fwd(const void* x, int dtype, int64_t N, int64_t H, int64_t W, int64_t C, int64_t Ho, int64_t Wo,
                            const void* add, void* y, mx_stream_t stream);
int mx_upsample_nearest_bwd(const void* gy, int dtype, int64_t N, int64_t H, int64_t W, int64_t C, int64_t Ho, int64_t Wo,
                            void* gx, mx_stream_t stream);

/* Train-mode BatchNorm2d around the conv (torch.nn.BatchNorm2d semantics, momentum 0.1,
 * unbiased running_var). finalize: reduce stats partials -> mean/invstd (f64 accumulation), fold
 * into scale/shift, update running stats. apply: y = act(x*scale + shift (+ residual)), act 0 none,
 * 1 relu, 2 leaky relu(0.2). bwd_reduce + bwd_apply: BN backward through the activation mask. */
int mx_bn_finalize(const float* stats, int64_t mblocks, int64_t K, int64_t count, const float* gamma,
                   const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                   float* mean_out, float* invstd_out, float* scale_out, float* shift_out, mx_stream_t stream);
/* Hot-path finalize: one launch (row-slice partials + the last block per 64-channel chunk finishes).
 * ws = mx_bn_finalize_workspace(mblocks, K) bytes; its first 256 bytes are arrival counters that
 * must be zero before the first use and are left zero by every launch, so one zero-filled scratch
 * serves all launches on a stream (use one scratch per concurrent stream). */
/* BN backward from column partials [2][mb][K] (mx_conv2d_dgrad_bnb): sums (dbeta, dgamma) and coef
 * as mx_bn_bwd_reduce_ex produces them. Workspace: mx_bn_finalize_workspace(mb, K), counters
 * zero-kept. */
int mx_bn_bwd_finalize(const float* part, int64_t mb, int64_t K, int64_t M, const float* mean, const float* invstd,
                       const float* gamma, float* sums, float* coef, void* ws, size_t ws_bytes, mx_stream_t stream);
/* RegionProposalNetwork.compute_loss over N*A anchors (objectness [n], deltas / targets [n][4] f32,
 * labels [n] (1 fg / 0 bg / -1), pos / neg sampler masks [n] u8): out[0] = mean BCE-with-logits over
 * the sampled anchors, out[1] = smooth-L1(beta) summed over the positives / number sampled,
 * out[2] = number sampled. Deterministic (fixed-order f64 finish). Workspace counters zero-kept. */
size_t mx_rpn_loss_workspace(int64_t n);
int mx_rpn_loss_fwd(const float* objectness, const float* deltas, const float* labels, const float* targets,
                    const uint8_t* pos, const uint8_t* neg, int64_t n, float beta, float* out, void* ws,
                    size_t ws_bytes, mx_stream_t stream);
/* Gradients of (out[0], out[1]) scaled by grad[0..1] (device) w.r.t. objectness and deltas. */
int mx_rpn_loss_bwd(const float* objectness, const float* deltas, const float* labels, const float* targets,
                    const uint8_t* pos, const uint8_t* neg, int64_t n, float beta, const float* out, const float* grad,
                    float* grad_objectness, float* grad_deltas, mx_stream_t stream);
/* fastrcnn_loss over R sampled RoIs: logits [R][ldl] (C classes), box regression [R][ldr] (4 per
 * class), labels [R] int64, targets [R][4]: out[0] = mean cross-entropy, out[1] = smooth-L1(beta) of
 * the labelled class's box over positive RoIs / R. Workspace: mx_rpn_loss_workspace(R). Backward:
 * grad_logits [R][C], grad_reg [R][4C] (dense) for upstream grad[0..1]. */
int mx_roi_loss_fwd(const float* logits, int64_t ldl, int C, const float* reg, int64_t ldr, const int64_t* labels,
                    const float* targets, int64_t R, float beta, float* out, void* ws, size_t ws_bytes,
                    mx_stream_t stream);
int mx_roi_loss_bwd(const float* logits, int64_t ldl, int C, const float* reg, int64_t ldr, const int64_t* labels,
                    const float* targets, int64_t R, float beta, const float* grad, float* grad_logits,
                    float* grad_reg, mx_stream_t stream);
size_t mx_bn_finalize_workspace(int64_t mblocks, int64_t K);
int mx_bn_finalize_ex(const float* stats, int64_t mblocks, int64_t K, int64_t count, const float* gamma,
                      const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                      float* mean_out, float* invstd_out, float* scale_out, float* shift_out, void* ws,
                      size_t ws_bytes, mx_stream_t stream);
/* Test-time BatchNorm adaptation for the eval forward (prediction-time BN, Nado et al. 2020; the blend
 * with a source prior is Schneider et al. 2020, eq. 1). The reference evaluates with the running
 * statistics only (evaluate_frcnn.py, model.eval()); this is an opt-in addition. One launch with the
 * grid, workspace (mx_bn_finalize_workspace(mblocks, K)) and zero-kept counters of mx_bn_finalize_ex.
 * Per channel, in f64, from the partials of this forward's `count` rows:
 *   m_b = sum z / count,  v_b = max(sum z^2 / count - m_b^2, 0)                  (biased variance)
 *   state null (batch mode): (m_t, v_t) = (m_b, v_b)
 *   state [3][K] f64 = (rows, mean, M2), zero at the start (stream mode), merged in place (Chan):
 *     d = m_b - mean, rows' = rows + count, mean' = mean + d*count/rows',
 *     M2' = M2 + v_b*count + d^2*rows*count/rows',  (m_t, v_t) = (mean', M2'/rows')
 *   a = prior / (prior + n_images),  mu = a*src_mean + (1-a)*m_t,  var = a*src_var + (1-a)*v_t
 *   mean_out = (float)mu, var_out = (float)var, invstd = (float)(1/sqrt(var + eps)),
 *   scale_out = gamma*invstd, shift_out = beta - (float)mu*scale_out     (as mx_bn_finalize_ex)
 * prior and n_images count images; n_images is the number of images behind (m_t, v_t), this forward
 * included (the caller keeps it: nothing is read back). gamma / beta nullable (1 / 0). src_mean and
 * src_var (the module's running statistics) are read only; no running statistic is written. Errors
 * (outputs untouched): prior < 0, prior + n_images <= 0, null src_mean / src_var, K > 4096, a short
 * workspace. */
int mx_bn_finalize_adapt(const float* stats, int64_t mblocks, int64_t K, int64_t count, const float* gamma,
                         const float* beta, float eps, const float* src_mean, const float* src_var, double prior,
                         double n_images, double* state /* nullable; [3][K] rows, mean, M2; updated in place */,
                         float* mean_out, float* var_out, float* scale_out, float* shift_out, void* ws, size_t ws_bytes,
                         mx_stream_t stream);
/* apply: x of xdtype, residual and y of ydtype (bf16 -> bf16, f32 -> bf16, f32 -> f32). */
int mx_bn_apply(const void* x, int xdtype, int64_t M, int64_t K, const float* scale, const float* shift,
                const void* residual, int act, void* y, int ydtype, mx_stream_t stream);
/* mx_bn_apply (f32, no residual) followed by mx_maxpool_fwd (k, stride, pad; no argmax) in one pass,
 * bit-identical to the two: y [N, Ho, Wo, C] = maxpool(act(z * scale + shift)). The ResNet stem's
 * bn1 -> relu -> maxpool (torchvision resnet.py _forward_impl, reached from train_frcnn_baseline.py:171)
 * when no gradient flows through them (frozen stem). */
int mx_bn_act_maxpool(const float* z, int64_t N, int64_t H, int64_t W, int64_t C, const float* scale, const float* shift,
                      int act, int k, int stride, int pad, float* y, mx_stream_t stream);
/* Hot-path backward: reduce_ex = one launch of per-row-block partials (no float atomics) whose last
 * block per 64-channel chunk does the f64 column reduce, writing sums[2][K] = (sum g, sum g*xhat) =
 * (dbeta, dgamma) and coef[3][K], the per-channel affine form dx = coef0*g + coef1*x + coef2;
 * workspace mx_bn_bwd_workspace bytes whose first 256 bytes are arrival counters (zero before first
 * use, left zero: see mx_bn_finalize_ex). apply_ex streams dx (and dres = g, nullable).
 * g = dy * act'(y); y may be null when act == 0. */
size_t mx_bn_bwd_workspace(int64_t M, int64_t K);
int mx_bn_bwd_reduce_ex(const void* dy, const void* y, const void* x, int dtype, int64_t M, int64_t K, int act,
                        const float* mean, const float* invstd, const float* gamma, void* ws, size_t ws_bytes,
                        float* sums, float* coef, mx_stream_t stream);
int mx_bn_bwd_apply_ex(const void* dy, const void* y, const void* x, int dtype, int64_t M, int64_t K, int act,
                       const float* coef, void* dx, void* dres, mx_stream_t stream);
/* Backward head of conv (+bias) (+act) (the ConvAct layers: RPN head convs, cls/bbox heads, FC6/FC7,
 * predictor): g[M][K8] (gdtype: bf16, or f32 for the bf16x3 path) = gy * act'(y) (columns K..K8-1 zero), db[K] f32 = column sums of the
 * unrounded g (nullable). gy, y: [M][K] of dtype MX_BF16 / MX_F32 (y nullable when act == 0).
 * ws = mx_act_bias_bwd_workspace(M, K) bytes with the zero-kept counters of mx_bn_finalize_ex
 * (needed only when db is given). */
size_t mx_act_bias_bwd_workspace(int64_t M, int64_t K);
int mx_act_bias_bwd(const void* gy, const void* y, int dtype, int64_t M, int64_t K, int64_t K8, int act,
                    void* g, int gdtype, float* db, void* ws, size_t ws_bytes, mx_stream_t stream);
/* Convenience forms (allocate per call): sums[2][K] is overwritten. */
int mx_bn_bwd_reduce(const uint16_t* dy, const uint16_t* y, const uint16_t* x, int64_t M, int64_t K, int act,
                     const float* mean, const float* invstd, float* sums, mx_stream_t stream);
int mx_bn_bwd_apply(const uint16_t* dy, const uint16_t* y, const uint16_t* x, int64_t M, int64_t K, int act,
                    const float* mean, const float* invstd, const float* gamma, const float* sums,
                    uint16_t* dx, uint16_t* dres /*nullable: grad of residual = masked dy*/,
                    mx_stream_t stream);

/* Multi-tensor SGD step (torch.optim.SGD semantics; the reference's SGD(lr 0.005, momentum 0.9,
 * weight_decay 5e-4), scripts/train_frcnn_baseline.py:149-153, step at :176): for each of `count`
 * f32 tensors (host arrays of device pointers / element counts), d = g + wd*p; buf = first[i] ? d :
 * momentum*buf + (1-dampening)*d; p -= lr * (nesterov ? d + momentum*buf : buf). One launch per 64
 * tensors. */
int mx_sgd_step(float* const* params, const float* const* grads, float* const* momentum_bufs,
                const int64_t* numels, const uint8_t* first, int64_t count, float lr, float momentum,
                float dampening, float weight_decay, int nesterov, mx_stream_t stream);
/* Multi-tensor AdamW step (torch.optim.AdamW semantics: decoupled decay, no amsgrad, no maximize; the
 * reference's AdamW(lr 1e-3, weight_decay 1e-4), train_restoration.py:246, step at :272): for each of
 * `count` f32 tensors (host arrays of device pointers / element counts), with steps[i] the tensor's step
 * number AFTER this step (>= 1),
 *   p *= 1 - lr*wd;  m += (1-beta1) * (g - m);  v = v*beta2 + (1-beta2) * (g*g);
 *   p -= lr / (1 - beta1^step) * (m / (sqrt(v) / sqrt(1 - beta2^step) + eps))
 * in this order. The constants are derived in double and rounded to f32 once; every f32 op rounds
 * once (no contraction), division and square root IEEE-rounded. One launch per 64 tensors. */
int mx_adamw_step(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                  const int64_t* numels, const int64_t* steps, int64_t count, double lr, double beta1, double beta2,
                  double eps, double weight_decay, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Restoration pre-pass on device (scripts/restore_testsets.py:53-79, restoration_net.py:44-106).
 *   reflect_pad_u8: cv2.copyMakeBorder(0, Hp-H, 0, Wp-W, BORDER_REFLECT), uint8 [B,H,W,C] -> [B,Hp,Wp,C]
 *   up_concat: ConvTranspose2d(2, s2) output held as [N,H,W,4*Cu] (channel = (i, j, co)) scattered to
 *              [N,2H,2W,Cu] and concatenated with skip [N,2H,2W,Cs] along channels (torch.cat dim=1)
 *   restore_finish: clamp(u8/255 + residual, 0, 1) * 255 -> clip -> truncate to uint8, cropped to H x W
 * ------------------------------------------------------------------------------------------- */
int mx_reflect_pad_u8(const uint8_t* src, int64_t B, int64_t H, int64_t W, int64_t C, int64_t Hp, int64_t Wp,
                      uint8_t* dst, mx_stream_t stream);
int mx_up_concat(const void* up, const void* skip, int dtype, int64_t N, int64_t H, int64_t W, int64_t Cu, int64_t Cs,
                 void* out, mx_stream_t stream);
/* Backward of mx_up_concat (U-Net training, train_restoration.py:199-205): gcat [N,2H,2W,Cu+Cs] ->
 * gup [N,H,W,4*Cu] and gskip [N,2H,2W,Cs] (NULL: skipped). */
int mx_up_concat_bwd(const void* gcat, int dtype, int64_t N, int64_t H, int64_t W, int64_t Cu, int64_t Cs, void* gup,
                     void* gskip, mx_stream_t stream);
int mx_restore_finish(const uint8_t* img_padded, int64_t B, int64_t Hp, int64_t Wp, const float* residual, int64_t H,
                      int64_t W, uint8_t* out, mx_stream_t stream);
/* mx_restore_finish under a per-image verdict (device int32 [B], as mx_degradation_stats_u8 writes it; csrc/
 * mx_gate.hip): for verdict[b] == 1 the bytes of mx_restore_finish, for 0 out[b] is the unpadded crop of
 * img_padded[b] (the image passes through). */
int mx_restore_finish_gated(const uint8_t* img_padded, int64_t B, int64_t Hp, int64_t Wp, const float* residual, int64_t H,
                            int64_t W, const int32_t* verdict, uint8_t* out, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * U-Net training loss L1 + weight * (1 - SSIM) (train_restoration.py:142-178: ssim() with an 11x11
 * Gaussian window, sigma 1.5, zero 'same' padding, C1 = 0.01^2, C2 = 0.03^2; CombinedLoss). Images
 * pred / target NHWC f32 [N,H,W,C] (the NCHW tensors of the reference in channels-last memory).
 *   mx_ssim_l1_fwd: out3[0] = mean SSIM, out3[1] = mean |pred - target|, out3[2] = out3[1] +
 *                   weight * (1 - out3[0]) (device floats). dmaps (nullable, 3 * N*H*W*C f64) receives
 *                   the per-pixel derivatives of the SSIM map the backward needs. Deterministic
 *                   (fixed-order f64 reduction); window sums in f64. Workspace mx_ssim_workspace().
 *   mx_ssim_l1_bwd: grad = gout[0] * (cs * d(sum SSIM)/d pred + cl * sign(pred - target)); for the
 *                   combined loss cs = -weight / numel, cl = 1 / numel; for mean SSIM cs = 1/numel, cl = 0.
 *   window odd <= 15, sigma > 0.
 * ------------------------------------------------------------------------------------------- */
size_t mx_ssim_workspace(int64_t N, int64_t H, int64_t W, int64_t C);
int mx_ssim_l1_fwd(const float* pred, const float* target, int64_t N, int64_t H, int64_t W, int64_t C, int window,
                   float sigma, float c1, float c2, float weight, float* out3, double* dmaps, void* ws, size_t ws_bytes,
                   mx_stream_t stream);
int mx_ssim_l1_bwd(const float* pred, const float* target, const double* dmaps, int64_t N, int64_t H, int64_t W,
                   int64_t C, int window, float sigma, const float* gout, float cs, float cl, float* grad,
                   mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Baseline JPEG decode, hybrid (replaces the PIL / cv2.imread JPEG decode of
 * coco_detection_dataset.py:23 (Image.open(...).convert("RGB")), restore_testsets.py:99 and
 * build_corrupted_testsets.py:139, all libjpeg(-turbo) ISLOW + fancy upsampling):
 *   mx_jpeg_parse         host: markers of a baseline (SOF0/SOF1) Huffman JPEG -> mx_jpeg_info
 *                         (MX_EUNSUPPORTED for progressive / arithmetic / lossless / CMYK / 4:4:0,
 *                         RGB-coded frames (libjpeg default_decompress_parms: no JFIF and Adobe
 *                         transform 0, or component ids 'R','G','B') and frames over 2^28 pixels;
 *                         MX_EINVAL for malformed headers: over-subscribed Huffman counts, undefined
 *                         quantisation tables, short segments).
 *   mx_jpeg_decode_coefs  host: entropy decoding (sequential bitstream; restart markers honoured)
 *                         into quantised coefficients, natural order, int16 [comp][by][bx][64].
 *   mx_jpeg_reconstruct   device: dequantisation + jpeg_idct_islow (jidctint.c integer IDCT) per
 *                         8x8 block into component planes (ws, mx_jpeg_workspace() bytes), then
 *                         h2v1 / h2v2 fancy upsampling (jdsample.c) and the YCbCr -> RGB tables of
 *                         jdcolor.c into out[height][width][3] uint8 (RGB, or BGR with bgr = 1 like
 *                         cv2.imread). Bit-exact with libjpeg-turbo's default decode.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t width, height, ncomp;       /* ncomp 1 (grey) or 3 (YCbCr) */
  int32_t h[3], v[3], tq[3];          /* sampling factors, quantisation table per component */
  int32_t hmax, vmax, mcux, mcuy;     /* MCUs across / down */
  int32_t bw[3], bh[3];               /* blocks per row / block rows of each component (MCU padded) */
  int32_t dw[3], dh[3];               /* downsampled_width / height (jdmaster.c) */
  int64_t coef_off[3], coef_total;    /* int16 offsets of each component's blocks; total int16s */
  int32_t restart_interval;
  int32_t scan_off;                   /* byte offset of the entropy-coded data */
  uint16_t qt[4][64];                 /* quantisation tables, natural order */
  uint8_t cid[3], td[3], ta[3];       /* component ids, DC / AC Huffman table of each component */
  uint8_t hbits[8][17], hval[8][256]; /* Huffman tables: 0-3 DC, 4-7 AC (BITS, HUFFVAL) */
  uint8_t hdef[8];
} mx_jpeg_info;
int mx_jpeg_parse(const uint8_t* data, int64_t n, mx_jpeg_info* info);
int mx_jpeg_decode_coefs(const uint8_t* data, int64_t n, const mx_jpeg_info* info, int16_t* coefs_host);
size_t mx_jpeg_workspace(const mx_jpeg_info* info);
int mx_jpeg_reconstruct(const int16_t* coefs, const mx_jpeg_info* info, void* ws, size_t ws_bytes, uint8_t* out,
                        int bgr, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Windowed reconstruct (the U-Net patch loader: train_restoration.py:63-111 keeps one patch_size
 * crop of each frame): the pixels of a window of the frame from the coefficients, with work and HBM
 * traffic proportional to the window. No workspace: no full-frame component plane is written.
 *   mx_jpeg_reconstruct_window  device: out[r][c][0..2] (uint8, rows out_row_bytes apart) for r < h,
 *                         c < w = full[y0 + r][x0 + (hflip ? w - 1 - c : c)], where full is what
 *                         mx_jpeg_reconstruct writes for the same coefs, info and bgr -- bit for
 *                         bit, for 4:4:4 / 4:2:2 / 4:2:0 / grey and any window inside the frame
 *                         (need not be MCU aligned; 1x1 is fine). out_row_bytes >= 3 * w lets a
 *                         patch go straight into slot b of a [B][S][S][3] batch; no byte outside the
 *                         h rows of 3 * w bytes is touched. One workgroup per 32x32 tile of the image
 *                         grid loads (16 B per lane) only the luma blocks of its part of the window
 *                         and the chroma blocks under it plus the one-sample halo of the fancy
 *                         upsampling, runs the islow IDCT with 8 lanes per block into LDS planes,
 *                         then upsamples, converts and stores. The fancy / replicate switch and the
 *                         edge clamps are the image's, never the window's. MX_EINVAL before any HIP
 *                         call for null pointers, an unparsed or inconsistent info, w <= 0 or
 *                         h <= 0, a window not inside [0, width) x [0, height), out_row_bytes <
 *                         3 * w, coefs not 16-byte aligned.
 *   mx_jpeg_window_cover  host: cover[c] = (bx0, by0, bx1, by1), high end exclusive: the blocks of
 *                         component c that hold a sample the window reads, halo included (all 0 for
 *                         the absent components of a grey frame). The function the kernel calls for
 *                         each tile's part of the window. MX_EINVAL as above.
 * ------------------------------------------------------------------------------------------- */
int mx_jpeg_reconstruct_window(const int16_t* coefs, const mx_jpeg_info* info, int x0, int y0, int w, int h, int hflip,
                               int bgr, uint8_t* out, int64_t out_row_bytes, mx_stream_t stream);
int mx_jpeg_window_cover(const mx_jpeg_info* info, int x0, int y0, int w, int h, int32_t cover[3][4]);

/* ---------------------------------------------------------------------------------------------
 * Entropy decoding on the device: the scan of a file mx_jpeg_parse accepts (1 or 3 components, any
 * accepted sampling, custom Huffman tables, restart intervals) -> the coefficients
 * mx_jpeg_decode_coefs produces, bit for bit, whenever the status word is 0. A Huffman stream
 * re-synchronises: a decoder started at a wrong bit falls into step with the true one after a few
 * symbols, so lanes decode fixed-size subsequences speculatively and a fix-up iteration makes every
 * lane's start state the true one (the exact sequential result, not an approximation).
 *   mx_jpeg_entropy_decode  device: scan_dev = the file's bytes from info->scan_off to its end
 *                         (nbytes of them, in HBM, any byte alignment) -> coefs_dev, int16
 *                         [comp][by][bx][64] natural order (coef_total of them, ready for
 *                         mx_jpeg_reconstruct) and *status_dev (one int32: 0, or MX_JPEG_ST_* bits).
 *                         Passes: (1) markers and FF 00 pairs per 4-KiB chunk, scans, compaction to the
 *                         unstuffed stream + restart-segment starts; (2) one lane per subsequence of
 *                         S bits walks from an assumed state and records its exit state; (3) lanes
 *                         re-walk from their predecessor's exit state to a fixed point: inside a
 *                         workgroup with barriers, across workgroups by further launches that exit at
 *                         once when the launch before changed no workgroup's last exit state (at most
 *                         workgroups - 1 of them; no workgroup waits on another); (4) scan of the blocks
 *                         completed per lane; (5) the output is cleared and every lane walks from its
 *                         true state storing AC values and DC differences; (6) per-component DC prefix
 *                         sums in 32 bits, reset at restart segments. No host synchronisation.
 *                         With a non-zero status the coefficients are unspecified (callers decode
 *                         that file with mx_jpeg_decode_coefs, which also defines what a damaged stream
 *                         decodes to). MX_EINVAL before any HIP call for null pointers, nbytes <= 0 or
 *                         >= 2^31, a short or misaligned (256 B) workspace, coefs_dev not 16-byte
 *                         aligned, a Huffman table the host decoder rejects.
 *   mx_jpeg_entropy_decode_workspace  bytes of ws for a scan of nbytes (0 for a bad info / nbytes).
 *   mx_jpeg_entropy_decode_set_subseq  S in bits: 64 (minimum) .. 65536, default 512; MX_EINVAL
 *                         outside. A process setting, results identical (tests run at the minimum,
 *                         where a 64x64 image has as many lanes as a 1333x800 one at the default).
 *   mx_jpeg_decode_coefs_chunked  host: the same passes run serially over the whole file `data`
 *                         (workgroups of 256 lanes emulated), sharing the per-symbol walk with the
 *                         kernels (csrc/mx_jpeg_walk.h). The CPU reference of the kernels, not a
 *                         product path. subseq_bits 0: the current setting.
 * ------------------------------------------------------------------------------------------- */
#define MX_JPEG_ST_CODE 1     /* a bit pattern that is no Huffman code */
#define MX_JPEG_ST_DC 2       /* DC size over 11 */
#define MX_JPEG_ST_RUN 4      /* AC run past coefficient 63 */
#define MX_JPEG_ST_SHORT 8    /* data exhausted or a marker reached before a segment's last MCU */
#define MX_JPEG_ST_RESTART 16 /* the number of restart markers does not fit the restart interval */
size_t mx_jpeg_entropy_decode_workspace(const mx_jpeg_info* info, int64_t nbytes);
int mx_jpeg_entropy_decode(const uint8_t* scan_dev, int64_t nbytes, const mx_jpeg_info* info, void* ws, size_t ws_bytes,
                           int16_t* coefs_dev, int32_t* status_dev, mx_stream_t stream);
int mx_jpeg_entropy_decode_set_subseq(int bits);
int mx_jpeg_decode_coefs_chunked(const uint8_t* data, int64_t n, const mx_jpeg_info* info, int subseq_bits,
                                 int16_t* coefs_host, int32_t* status);

/* ---------------------------------------------------------------------------------------------
 * Baseline JPEG encode (replaces the PIL / cv2.imwrite JPEG encode of build_corrupted_testsets.py
 * and restore_testsets.py). Byte-identical to libjpeg-turbo behind PIL's
 * Image.save(format="JPEG", quality=q, subsampling=s): SOI, JFIF APP0, two DQT, SOF0, four DHT (the
 * T.81 K.3-K.6 tables), SOS, the scan, EOI. The encoder reuses mx_jpeg_info.
 *   mx_jpeg_encode_info   host: geometry (as mx_jpeg_parse fills it), component ids 1,2,3, quantisation
 *                         tables 0,1,1 = the Annex K tables scaled like jpeg_quality_scaling, the
 *                         standard Huffman tables; scan_off = the header's length. subsampling in
 *                         PIL's numbering: 0 = 4:4:4, 2 = 4:2:0. MX_EINVAL for another subsampling or
 *                         a quality outside 1..100, MX_EUNSUPPORTED over 65535 a side or 2^28 pixels.
 *   mx_jpeg_write_header  host: the marker segments up to and including SOS into out[cap]; *n = bytes
 *                         (MX_EINVAL and the needed *n when cap is short; nothing past cap is written).
 *   mx_jpeg_scan_bound    host: worst-case bytes of the entropy-coded segment of this geometry.
 *   mx_jpeg_encode_coefs  host: sequential Huffman coding (jchuff.c) of natural-order int16
 *                         coefficients [comp][by][bx][64] with the tables of `info` (parsed or from
 *                         mx_jpeg_encode_info; 4:2:0 / 4:2:2 / 4:4:4 / grey): interleaved MCUs, DC
 *                         differences per component, ZRL / EOB, 0xFF 0x00 stuffing, the last byte padded
 *                         with ones. Writes the entropy-coded segment only (the caller appends EOI).
 *                         MX_EUNSUPPORTED for restart_interval != 0; MX_EINVAL when cap is short (never
 *                         written past) or a coefficient has no code. The CPU reference of, and the
 *                         fallback for, mx_jpeg_entropy.
 *   mx_jpeg_forward       device: uint8 pixels [height][width][3] (RGB, or BGR with bgr = 1) ->
 *                         quantised coefficients in that layout, dummy blocks included: colour
 *                         conversion, edge replication, h2v2 chroma downsampling, jpeg_fdct_islow and
 *                         quantisation fused per MCU strip through LDS. 3 components, 4:4:4 or 4:2:0
 *                         (MX_EUNSUPPORTED otherwise). coefs_dev 16-byte aligned, coef_total int16s.
 *   mx_jpeg_entropy       device: the same bytes as mx_jpeg_encode_coefs into out_dev[out_cap], the
 *                         length into *nbytes_dev (one int64; -1 when a coefficient has no code; a
 *                         length over out_cap means the output was cut at out_cap). Multi-launch
 *                         passes (bit counts, scans, bit scatter, 0xFF stuffing), no host
 *                         synchronisation; ws: mx_jpeg_entropy_workspace() bytes, 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
int mx_jpeg_encode_info(int width, int height, int quality, int subsampling, mx_jpeg_info* out);
int mx_jpeg_write_header(const mx_jpeg_info* info, uint8_t* out, int64_t cap, int64_t* n);
int64_t mx_jpeg_scan_bound(const mx_jpeg_info* info);
int mx_jpeg_encode_coefs(const mx_jpeg_info* info, const int16_t* coefs_host, uint8_t* out, int64_t cap, int64_t* n);
int mx_jpeg_forward(const uint8_t* img, int bgr, const mx_jpeg_info* info, int16_t* coefs_dev, mx_stream_t stream);
size_t mx_jpeg_entropy_workspace(const mx_jpeg_info* info);
int mx_jpeg_entropy(const int16_t* coefs_dev, const mx_jpeg_info* info, void* ws, size_t ws_bytes, uint8_t* out_dev,
                    int64_t out_cap, int64_t* nbytes_dev, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * JPEG compression as a corruption: out[b] = the pixels libjpeg-turbo decodes from the file it writes
 * for img[b] at quality_host[b] -- PIL's Image.open(BytesIO(save(img[b], "JPEG", quality, subsampling)))
 * .convert("RGB"), bit for bit; with bgr = 1 both img and out are BGR. img, out: uint8 [B][H][W][3],
 * contiguous, out not overlapping img. quality_host[b] in 1..100, or 0: out[b] is left untouched (a
 * batch in which only some images get this corruption). subsampling 0 (4:4:4) or 2 (4:2:0), PIL's
 * numbering as in mx_jpeg_encode_info, whose quantisation tables the kernel derives from the quality.
 * Two launches per 64 compressed images: the pixel stage of mx_jpeg_forward continued through
 * dequantisation and jpeg_idct_islow inside the workgroup (no coefficient reaches memory) into the
 * component planes of ws, then chroma upsampling + YCbCr -> RGB as in mx_jpeg_reconstruct. ws:
 * mx_corrupt_jpeg_workspace() bytes (B x the planes of one image; 0 for a bad shape), 8-byte aligned.
 * Stream-ordered, no host synchronisation, no allocation. Every argument check precedes the first
 * launch: MX_EINVAL for a null pointer, a quality outside 0..100, another subsampling, out == img or
 * overlapping it, a short workspace, a side over 65535 or more than 2^28 pixels.
 * ------------------------------------------------------------------------------------------- */
size_t mx_corrupt_jpeg_workspace(int64_t B, int64_t H, int64_t W, int subsampling);
int mx_corrupt_jpeg_u8(const uint8_t* img, int64_t B, int64_t H, int64_t W, const int32_t* quality_host,
                       int subsampling, int bgr, void* ws, size_t ws_bytes, uint8_t* out, mx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * COCOeval (bbox) on the device: pycocotools' COCOeval.evaluate (computeIoU + evaluateImg) and
 * accumulate, as train_frcnn_baseline.py:92-96 and eval_all.py:131-156 call them. f64 throughout, every
 * operation rounded once and in the host code's order (maskApi bbIou; mx_det/coco.py is the restated
 * host form): the outputs are bit-identical to it.
 *   Layout. A segment is one (image, category) pair with at least one GT or one detection; the S
 *   segments are ordered by (category index, image index). Detections [ND] are sorted by (category,
 *   image, score descending, ties in result order) and each segment holds at most maxDets[-1] of them;
 *   GT [NG] by (category, image, annotation order). dt_off / gt_off [S+1] int32 are the segments'
 *   offsets into them. dt_xywh [ND][4], dt_area [ND] (w*h); gt_xywh [NG][4], gt_area [NG] (the
 *   annotation's area field), gt_crowd [NG] u8, gt_id [NG]. area_rng [A][2], iou_thr [T], rec_thr [R]
 *   (ascending) f64 and max_dets [M] int32 are device arrays holding the host's parameter values.
 *   max_g / max_d: upper bounds on one segment's GT / detection count (NG / ND are always safe).
 *   mx_coco_match   one launch, one wave per (segment, area range, threshold): a GT is ignored when
 *                   crowd or its area is outside [a0, a1]; detections in score order take the
 *                   still-free GT (crowd GTs stay free) of highest IoU >= min(t, 1 - 1e-10), non-ignored
 *                   GTs before ignored ones, the later annotation among equal IoUs.
 *                   dtm [A][T][ND] = the matched GT's id (0: none), dt_ig [A][T][ND] u8 = the matched
 *                   GT's ignore flag, or 1 when dtm == 0 and the detection's area is outside the range,
 *                   gt_ig [A][NG] u8. A 0/0 IoU never matches. MX_EUNSUPPORTED for max_g > 61440 (one
 *                   flag byte per GT of a segment in LDS); a segment found above max_g on the device
 *                   gets dtm = -1 rather than a truncated match.
 *   mx_coco_accumulate  two launches. perm [ND] int64: for each category's range cat_dt_off[k] ..
 *                   cat_dt_off[k+1] of the detections, their indices by score descending (stable);
 *                   dt_score [ND]; cat_gt_off [K+1] the categories' GT ranges. For each (k, a, m, t) over
 *                   the detections of rank < max_dets[m] in their segment: tp = dtm != 0 && !dt_ig,
 *                   fp = dtm == 0 && !dt_ig, running sums, recall tp / npig, precision
 *                   tp / (fp + tp + 2^-52) made non-increasing from the right, sampled with its score
 *                   at searchsorted(recall, rec_thr, left) (0 past the last detection).
 *                   precision / scores [T][R][K][A][M], recall [T][K][A][M]; every entry is written,
 *                   -1 where the category has no non-ignored GT. R <= 2048. Workspace
 *                   mx_coco_accumulate_workspace(ND).
 * ------------------------------------------------------------------------------------------- */
int mx_coco_match(const double* dt_xywh, const double* dt_area, const int32_t* dt_off, int64_t ND,
                  const double* gt_xywh, const double* gt_area, const uint8_t* gt_crowd, const int64_t* gt_id,
                  const int32_t* gt_off, int64_t NG, int64_t S, const double* area_rng, int64_t A,
                  const double* iou_thr, int64_t T, int64_t max_g, int64_t max_d, int64_t* dtm, uint8_t* dt_ig,
                  uint8_t* gt_ig, mx_stream_t stream);
size_t mx_coco_accumulate_workspace(int64_t ND);
int mx_coco_accumulate(const int64_t* dtm, const uint8_t* dt_ig, const uint8_t* gt_ig, const double* dt_score,
                       const int64_t* perm, const int32_t* dt_off, int64_t S, int64_t ND, int64_t NG,
                       const int32_t* cat_dt_off, const int32_t* cat_gt_off, int64_t K, int64_t A, int64_t T,
                       const int32_t* max_dets, int64_t M, const double* rec_thr, int64_t R, double* precision,
                       double* scores, double* recall, void* ws, size_t ws_bytes, mx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
