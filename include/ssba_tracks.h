/*
 * ssba_tracks.h -- C ABI of libssba_tracks.so: sparse stereo feature tracks from raw 8-bit frames.
 *
 * The sparse branch (ssba_frontend_vo, ssba_add_stereo_observations; include/ssba.h) starts at rows [k, j, u, v, d] with
 * landmark ids.  The reference's own producer of such rows is its stereo-odometry node,
 * ros/src/ceres_slam/src/sparse_stereo_odometry_node.cpp:127-216: detect and describe in the left and right image, match left
 * to right with a cross-checked Hamming matcher (cv::BFMatcher(NORM_HAMMING, true)), keep pairs with |dy| < 5 and
 * x_right < x_left, match the survivors' left descriptors from frame to frame with the same matcher.  This library does that
 * on the device, from a stack of frames to the arrays ssba_frontend_vo takes, stated entirely in integers: the yardstick is
 * the numpy statement tests/tracks_reference.py, which the device equals to the bit.  OpenCV can be neither built nor run
 * where this library is tested, so parity with cv::ORB / cv::BFMatcher is UNPINNED; "this library's own rule" marks each place
 * where the arithmetic departs from the node on purpose.
 *
 * It is a library of its own: it shares no state with a solver handle and exports nothing but the names below.  Status codes
 * are ssba_status values (include/ssba.h is included for that enum only); the last-error string is this library's own.
 *
 * The arithmetic
 *   detector    the segment test on the 16-pixel Bresenham ring of radius 3 around a centre c, ring pixel i at (dx, dy) =
 *                   (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3)
 *               with values I_0 ... I_15.  An arc is 9 consecutive ring pixels, i ... i + 8 with indices wrapping 15 -> 0; there
 *               are 16.  s = max(0, max over arcs of min (I_i - c), max over arcs of min (c - I_i)): the largest threshold at
 *               which the segment test still holds, plus one.  A pixel is a candidate when s > fast_threshold and it lies
 *               at least SSBA_TRACK_BORDER = 15 pixels from every edge (13 for the descriptor's offsets plus 2 for its box), i.e.
 *               15 <= x < cols - 15 and 15 <= y < rows - 15.  Every other pixel has score 0.
 *   suppression 3 x 3: a candidate p survives if for each of its eight neighbours q  s(p) > s(q), or s(p) == s(q) and the
 *               row-major index of p is smaller than that of q.
 *   selection   at most max_features per image: the highest scores; among equal scores at the cut the smallest row-major
 *               indices.  The kept keypoints are output in ROW-MAJOR order, not by score (this library's own rule: a position
 *               that a prefix sum gives, no sort).
 *   descriptor  BRIEF-256 without orientation (this library's own rule: consecutive frames of a rig barely rotate, and the
 *               left and right image of a rectified rig do not at all; ORB's steering and pyramid are out of scope).  bit i = 1
 *               when box(p + a_i) < box(p + b_i), box(q) = the sum of the 5 x 5 pixels around q, an integer, never divided.
 *               The 256 pairs (a_i, b_i) in [-13, 13]^2 are this project's own, NOT OpenCV's table:
 *                   s = 20161021;   draw(): s = (s * 1103515245 + 12345) mod 2^31, return ((s >> 16) mod 27) - 13
 *                   pair i = (ax, ay, bx, by) = four draws in this order, drawn again while a_i == b_i
 *               tools/brief_pattern.py writes them to csrc/ssba_brief_pattern.h.  A descriptor is 8 uint32 words, bit i at
 *               word i / 32, position i % 32.
 *   matching    of a set A against a set B under a gate, cross-checked: for each a the best b minimises the Hamming distance
 *               over the b that pass the gate with a, the smallest index on ties; the best a of each b likewise; (a, b) is a
 *               match when each is the other's best and the distance <= max_hamming.  The gate is applied INSIDE the search
 *               (this library's own rule: the node filters after matching, which discards a feature whose global best lies
 *               off the epipolar line).
 *                   SSBA_TRACK_GATE_NONE      every pair passes
 *                   SSBA_TRACK_GATE_STEREO    A left, B right: |y_a - y_b| < stereo_max_dy (node :157) and 0 < x_a - x_b <= max_disparity
 *                   SSBA_TRACK_GATE_TEMPORAL  |x_a - x_b| <= temporal_radius and |y_a - y_b| <= temporal_radius; radius 0: no gate
 *   observation (u, v, d) = (x_l, y_l, x_l - x_r) as doubles for every stereo match of a frame (a "survivor"), in keypoint order.
 *               With a disp16 stack (the format ssba_stereo_sgbm_batch writes) the right images are not used:
 *               d = disp16[y][x] / 16.0, and a keypoint whose disp16 is <= 0 (invalid for min_disparity 0, or no positive
 *               depth) is dropped.  A matcher run with min_disparity >= 2 marks invalid pixels with a positive value; such a map
 *               must be masked by the caller.
 *   tracks      only survivors take part (node :170-186).  Frame 0's survivors get ids 0, 1, ... in keypoint order; in frame k a
 *               survivor matched (temporal gate, A = survivors of frame k - 1, B = those of frame k, left descriptors) to a
 *               survivor of frame k - 1 inherits its id, every other survivor gets the next free id in keypoint order.  Then
 *               the observations of tracks shorter than min_track_length are removed and the ids renumbered densely in order of
 *               first appearance.
 * No floating point is used before the final conversion of (u, v, d).  Every position in an output comes from a prefix sum, so
 * two runs give the same bytes.
 *
 * Sub-pixel refinement (ssba_track_refine, ssba_track_sequence_subpixel; the numpy statement is tests/tracks_refine_reference.py)
 *   Every observation of a track becomes the position of ONE template in that image: the 15 x 15 patch around the track's first
 *   observation, its anchor.  Positions are int32 in units of 1/256 pixel ("q8").
 *   template    anchor at whole pixel (ax, ay) of image A, offsets i, j in [-7, 7]:  T(i,j) = A[ay+j][ax+i],
 *               gx = A[ay+j][ax+i+1] - A[ay+j][ax+i-1], gy = A[ay+j+1][ax+i] - A[ay+j-1][ax+i]: twice the central difference,
 *               never divided.  In x-only mode gy = 0.  H11 = sum gx^2, H12 = sum gx gy, H22 = sum gy^2, integers.  An anchor
 *               whose 17 x 17 support leaves A (ax < 8, ax + 8 >= cols, likewise in y) has status EDGE.
 *   evaluation  at p = (px, py) in the target image B, for every (i, j):  X = px + 256 i, x0 = X >> 8 (the floor), fx = X & 255,
 *               y0 and fy likewise from py + 256 j;
 *                   S = (256-fx)(256-fy) B[y0][x0] + fx (256-fy) B[y0][x0+1] + (256-fx) fy B[y0+1][x0] + fx fy B[y0+1][x0+1]
 *                   e = S - 65536 T,   bx = sum gx e,   by = sum gy e   (int64, |b| < 2^41),   sad = (sum |e|) >> 16.
 *               If any x0 < 0, y0 < 0, x0 + 1 >= cols or y0 + 1 >= rows the status is EDGE and nothing is summed.
 *   step        det = H11 H22 - H12^2 in int64 (below 2^53, so its conversion to double is exact); det <= 0 is FLAT.  The only
 *               floating point: IEEE doubles, round to nearest, no contraction, every operand converted from its integer first
 *               and every product rounded before the subtraction,
 *                   nx = H22 bx - H12 by,   ny = H11 by - H12 bx,   dx = rint(nx / (det 128)),   dy = rint(ny / (det 128)).
 *               x-only mode: H11 <= 0 is FLAT, dx = rint(bx / (H11 128)), dy = 0.  Then p <- p - (dx, dy), exactly (a step too
 *               large for an int32 is FAR).  1/128 = 2 * 256 / 65536: the doubled gradients, the q8 unit, the 65536 of S.
 *   control     sad = 0;  then up to `iterations` times:  EDGE if the window at p leaves B;  FLAT;  evaluate;  step;
 *               max(|px - px_0|, |py - py_0|) > 256 max_shift is FAR;  max(|dx|, |dy|) <= 1 is convergence (the step has been
 *               applied, sad is that of the evaluation just made).  `iterations` evaluations without convergence: ITERATIONS.
 *               Converged with max_sad > 0 and sad > max_sad: SAD (max_sad 0: no such gate).  Otherwise OK.
 *               The position returned is p when the status is OK and the start otherwise; sad is that of the last evaluation
 *               made, 0 when there was none.
 *   sequence    launches, survivors and ids as ssba_track_sequence.  The anchor of an id is the survivor that was issued it.
 *               Per survivor at keypoint (x, y) with disparity d16 / 16 in frame f:  (u, v) = (256 x, 256 y) exactly when the
 *               survivor is its own anchor, else the 2-D refinement in left image f started there.  With right images the right
 *               position x_r is refined in x only in right image f, against the same (left) template, from u - 16 d16 on the
 *               row v (a q8 row: the refined one), and d = u - x_r; d <= 0 is DISPARITY.  With a disp16 stack only the left
 *               position is refined and d = 16 d16.  A survivor whose status is not OK is dropped: it counts in *num_dropped
 *               and its track is one observation shorter; the track keeps its other observations and its template, also when
 *               the dropped one is the anchor.  Pruning by min_track_length acts on the remaining lengths, ids are renumbered
 *               in id order, and (u, v, d) = q8 / 256.0.
 *
 * Streaming (the ssba_track_stream_ calls; the numpy statement is tests/tracks_stream_reference.py)
 *   The node this library restates gets one stereo pair per callback and keeps the previous pair's keypoints and descriptors
 *   (sparse_stereo_odometry_node.cpp:303-308).  A stream is that mode: a handle whose state stays on the device, frames pushed one
 *   by one, the work of a push independent of how many frames came before.
 *   state       the previous frame's survivors (count, positions, descriptors, issued ids), the running id, and a ring of the last
 *               `window` frames with, per survivor slot: the issued id, the slot of the frame before it inherited from (or none),
 *               the kept flag and the observation (whole pixel: x, y, d16; refined: u, v, d in q8).  With refinement also the
 *               ANCHOR PATCH of every survivor's track: the 17 x 17 bytes around the anchor, everything the template reads
 *               (a keypoint keeps 15 pixels from every edge, so the patch is inside its image).  An inheriting survivor carries
 *               its predecessor's patch on, a survivor that is issued an id cuts its own.
 *   push        features, stereo survivors and the temporal match of the new pair exactly as in the sequence calls; ids as the
 *               sequence calls issue them BEFORE pruning, the fresh ones counted on from the stream's running id: global to
 *               the stream, never renumbered, never pruned by min_track_length.  With refinement every survivor is placed as
 *               in "sequence" above against its track's patch; one whose status is not OK is dropped from the outputs and
 *               counts in *num_dropped, but stays in the state, so the next frame can still inherit its id and its patch (the
 *               sequence calls link before they refine, too).
 *   window      over the last `frames` pushed frames: a survivor of the oldest frame starts a track, a later survivor continues
 *               the track of the slot it inherited from or starts one.  A track's length is the number of its kept
 *               observations inside the window; tracks shorter than min_track_length go; the new ids are dense in the order of
 *               each track's first survivor in the window (frame, then keypoint slot; a dropped survivor counts for the order,
 *               not for the length).
 *   Two consequences, which the tests hold the device to:
 *   1. Whole pixel: after any number of pushes, a window over W frames equals ssba_track_sequence on those same W frames byte
 *      for byte, because the features, stereo survivors and temporal matches of a frame pair do not depend on history.
 *   2. Sub-pixel: a window over W frames equals ssba_track_sequence_subpixel over ALL frames since the stream began, restricted
 *      to the last W frames and then pruned and renumbered by the window rule.  With W = the number of pushed frames that is
 *      ssba_track_sequence_subpixel's output byte for byte.  With a shorter window it differs from the batch call on those W
 *      frames on purpose: the template is the track's first patch, not the window's.
 *   launches    per push, whatever came before: 4 for the features, k_tr_best left-right (right images only), k_tr_stereo,
 *               k_tr_best against the frame before (not on the first push), k_ts_link, with refinement k_ts_carry and
 *               k_ts_refine, k_ts_emit: 9 with right images (11 refined), one fewer with disp16 maps and on the first push.
 *               Per window call: 1, k_ts_window, whatever `frames`.  A push synchronises once.
 *   refusals    SSBA_ERR_INVALID_ARGUMENT before a device is looked for: NULL arguments; rows or cols outside 31 ... 8192; every
 *               parameter refusal above; window < 1 or > SSBA_TRACK_STREAM_MAX_WINDOW; both or neither of right / disp16; a push
 *               with the other disparity source than the stream's first; frames < 1 or above min(window, pushed frames); after
 *               the work, a capacity below the number of observations (the message names it; nothing is written).
 *               SSBA_ERR_STATE: a push when fewer than max_features ids are left below 2^32 - 1.
 *   use         a stream is one caller's: no two calls on the same stream may run at the same time (different streams may).  After
 *               a push or a window call that returned SSBA_ERR_HIP the device's state may be ahead of the host's, so the stream
 *               is dead: every later push or window call on it is SSBA_ERR_STATE, and only destroying it remains.
 *
 * Odometry (ssba_track_stream_enable_odometry, ssba_track_stream_pose, ssba_track_relative_pose; the statement is
 * tests/tracks_odometry_reference.py)
 *   The second half of the node's callback (sparse_stereo_odometry_node.cpp:176-301): the matches to the previous frame are
 *   triangulated, a 3-point RANSAC gives T_k_km1 and the inliers, a two-view solve over the inliers refines it, and the pose is
 *   chained.  A stream with odometry enabled does this inside every push, on the device, within the push's one synchronisation
 *   and one download.  Poses are [t | R row-major] with p_k = R p_km1 + t, the convention of ssba_frontend_vo;
 *   T_k_0 = T_k_km1 o T_km1_0 and T_0_0 = first_pose.
 *   matches     the ids present in both this push's and the previous push's outputs, in this push's order (the kept survivors
 *               whose id was inherited from a kept survivor), with exactly the (u, v, d) doubles those pushes returned: a caller
 *               can rebuild the list.  Both sides are triangulated by StereoCamera::triangulate,
 *               (x, y, z) = b / d ((u - cu), (v - cv) fu / fv, fu).
 *   draws       this library's own rule (the node's mt19937 stream needs n on the host): mix(x) is the 32-bit mixer
 *                   x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *               and hypothesis h of H in frame f (the index of the pushed frame, 0 for the first) uses the counter
 *               c = 3 (f H + h) mod 2^32:  i0 = mix(c) % n;  i1 = mix(c + 1) % (n - 1), plus 1 if >= i0;
 *               i2 = mix(c + 2) % (n - 2), plus 1 if >= min(i0, i1), then plus 1 if >= max(i0, i1).  Distinct by construction.
 *   hypotheses  the 3-point alignment and the inlier test (squared stereo reprojection error < ransac_threshold,
 *               point_cloud_aligner.cpp:117-124) are those of ssba_frontend_vo, the same source text.  The first hypothesis with
 *               the largest count wins; the inlier flags are the winner's.
 *   refinement  the node's two-view problem (:236-285) with the gauge fixed: pose k - 1 constant at the identity, pose k free
 *               from the RANSAC pose, one free point per inlier from its triangulation in frame k - 1, two
 *               StereoReprojectionError blocks per point with stiffness I / sqrt(observation_variance), no loss, the pose
 *               updated by exp(eps) T.  Levenberg-Marquardt exactly as oracle/ssba_oracle.c states it under orc_default_options
 *               with max_num_iterations = refine_iterations (Jacobi scaling, the diagonal clamps, the radius rule, every
 *               termination).  The points are eliminated in closed form, leaving one 6 x 6 system.  All fp64; every sum runs
 *               over the inliers in a fixed order without floating-point atomics, so two runs give the same bytes.
 *   status      SSBA_TRACK_POSE_OK; _FIRST_FRAME: the identity, T_k_0 = first_pose; _FEW_MATCHES: fewer than 3 matches, the
 *               identity, the chain continues; _FEW_INLIERS: the winner has fewer than 3 inliers, its pose stands without a
 *               refinement (the identity when no hypothesis has an inlier); _NUMERICAL: the refinement met a non-finite cost or
 *               five invalid steps in a row, the RANSAC pose stands.
 *   launches    per push with odometry 4 more than without: k_od_match, k_od_align, k_od_score, k_od_solve (2 more on the
 *               first push: k_od_match, k_od_solve).  No further synchronisation, no allocation, still one download: the push
 *               output block grows by the pose block.  A stream that does not enable odometry launches, allocates and returns
 *               what it did before.
 *   refusals    SSBA_ERR_INVALID_ARGUMENT before a device is looked for: NULL arguments; ransac_iterations outside 1 ... 4096;
 *               a non-positive (or non-finite) ransac_threshold, observation_variance, fu, fv or b; refine_iterations above
 *               1024; n above 4096.  SSBA_ERR_STATE: enabling odometry after the first push or twice; ssba_track_stream_pose
 *               on a stream without odometry or before its first push.
 *
 * SSBA_ERR_INVALID_ARGUMENT, with a message and before a device is looked for: a NULL input or output; both or neither of
 *   right / disp16; frames < 1 or > 32767 (n likewise, up to 65535); rows or cols < 31 or > 8192; max_features outside
 *   1 ... 4096; fast_threshold outside 0 ... 254; max_hamming outside 0 ... 256; a negative stereo_max_dy, max_disparity or
 *   temporal_radius; min_track_length < 1; an unknown gate; na or nb > 65535.  After the work: a capacity below the number of
 *   observations (the message names the number needed; nothing is written).  The refinement calls add: NULL refine
 *   parameters; iterations outside 1 ... 64; max_shift outside 1 ... 8; a negative max_sad; an item whose anchor or target
 *   image index is not below n; an item whose mode is neither 0 nor 1.
 * All calls are synchronous: host arrays in and out, the work on a pooled stream.
 */
#ifndef SSBA_TRACKS_H_
#define SSBA_TRACKS_H_

#include "ssba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSBA_TRACK_BORDER 15
#define SSBA_TRACK_MAX_FEATURES 4096
#define SSBA_TRACK_DESC_WORDS 8
#define SSBA_TRACK_GATE_NONE 0
#define SSBA_TRACK_GATE_STEREO 1
#define SSBA_TRACK_GATE_TEMPORAL 2

/* ssba_track_default_params: fast_threshold 20, max_features 1000, stereo_max_dy 5, max_disparity 128, max_hamming 64,
 * temporal_radius 0, min_track_length 2 */
typedef struct {
    int32_t fast_threshold, max_features, stereo_max_dy, max_disparity, max_hamming, temporal_radius, min_track_length;
} ssba_track_params;
SSBA_API void ssba_track_default_params(ssba_track_params *params);

/* Detector and descriptor alone over a stack of n images of rows x cols: count[n]; xy (n * max_features * 2: x, y),
 * score (n * max_features) and desc (n * max_features * 8) hold image k's keypoints from slot k * max_features on, zeros behind
 * the count.  Four launches whatever n. */
SSBA_API int ssba_track_features(const uint8_t *images, uint32_t n, uint32_t rows, uint32_t cols, const ssba_track_params *params, int device,
                                 uint32_t *count, uint16_t *xy, uint8_t *score, uint32_t *desc);

/* The matcher alone: match_a[i] = the index in B of a_i's match or -1, dist_a[i] its Hamming distance or -1.  desc_a / xy_a
 * may be NULL when na = 0, and likewise for B. */
SSBA_API int ssba_track_match(const uint32_t *desc_a, const uint16_t *xy_a, uint32_t na, const uint32_t *desc_b, const uint16_t *xy_b, uint32_t nb,
                              int gate, const ssba_track_params *params, int device, int32_t *match_a, int32_t *dist_a);

/* Everything: left holds `frames` images, then exactly one of right (as many) and disp16 (as many maps, int16) is given.
 * Outputs in ssba_frontend_vo's input format: state_start (frames + 1), point_id and uvd (3 per observation) with room for
 * `capacity` observations, *num_observations, *num_points.  The number of launches does not depend on `frames`. */
SSBA_API int ssba_track_sequence(const uint8_t *left, const uint8_t *right, const int16_t *disp16, uint32_t frames, uint32_t rows, uint32_t cols,
                                 const ssba_track_params *params, int device, uint64_t capacity, uint32_t *state_start, uint32_t *point_id,
                                 double *uvd, uint64_t *num_observations, uint32_t *num_points);

#define SSBA_TRACK_REFINE_OK 0
#define SSBA_TRACK_REFINE_EDGE 1
#define SSBA_TRACK_REFINE_FLAT 2
#define SSBA_TRACK_REFINE_FAR 3
#define SSBA_TRACK_REFINE_ITERATIONS 4
#define SSBA_TRACK_REFINE_SAD 5
#define SSBA_TRACK_REFINE_DISPARITY 6
#define SSBA_TRACK_REFINE_2D 0
#define SSBA_TRACK_REFINE_X_ONLY 1

/* ssba_track_default_refine_params: iterations 10, max_shift 4 (pixels), max_sad 0 (no gate) */
typedef struct {
    int32_t iterations, max_shift, max_sad;
} ssba_track_refine_params;
SSBA_API void ssba_track_default_refine_params(ssba_track_refine_params *params);

/* The refinement alone over a stack of n images: item k is 7 int32 = anchor image, ax, ay, target image, x0_q8, y0_q8, mode
 * (SSBA_TRACK_REFINE_2D or _X_ONLY).  Per item: xy_q8 (2 int32: the position, the start when the status is not OK), status
 * (SSBA_TRACK_REFINE_OK ... _SAD; _DISPARITY arises in the sequence only) and sad.  items and the outputs may be NULL when
 * num_items = 0, which is SSBA_OK without a launch.  One launch whatever num_items. */
SSBA_API int ssba_track_refine(const uint8_t *images, uint32_t n, uint32_t rows, uint32_t cols, const int32_t *items, uint32_t num_items,
                               const ssba_track_refine_params *refine_params, int device, int32_t *xy_q8, int32_t *status, uint32_t *sad);

/* ssba_track_sequence with sub-pixel observations: the same arguments, then the refinement's parameters and *num_dropped, the
 * number of survivors whose refinement did not end OK.  Two launches more than ssba_track_sequence, whatever `frames`. */
SSBA_API int ssba_track_sequence_subpixel(const uint8_t *left, const uint8_t *right, const int16_t *disp16, uint32_t frames, uint32_t rows, uint32_t cols,
                                          const ssba_track_params *params, int device, uint64_t capacity, uint32_t *state_start, uint32_t *point_id,
                                          double *uvd, uint64_t *num_observations, uint32_t *num_points,
                                          const ssba_track_refine_params *refine_params, uint64_t *num_dropped);

/* ---- streaming ---------------------------------------------------------------------------------------------------------- */
#define SSBA_TRACK_STREAM_MAX_WINDOW 256

typedef struct ssba_track_stream ssba_track_stream;

/* A stream for frames of rows x cols.  refine_params NULL: whole-pixel observations; otherwise sub-pixel ones.  window: how many
 * of the most recent frames ssba_track_stream_window can cover, 1 ... SSBA_TRACK_STREAM_MAX_WINDOW.  All device and pinned host
 * memory is allocated here (about 10 images, 64 bytes per keypoint slot and per window frame, 1 KiB per keypoint slot), none per
 * push; the stream holds one pooled stream until it is destroyed. */
SSBA_API int ssba_track_stream_create(uint32_t rows, uint32_t cols, const ssba_track_params *params, const ssba_track_refine_params *refine_params,
                                      uint32_t window, int device, ssba_track_stream **stream);

/* One stereo pair: the left image and exactly one of right / disp16, the same one in every push of a stream.  track_id and uvd
 * (3 per observation) MUST have room for max_features entries: the frame's kept survivors in keypoint order with their issued
 * ids.  *num_dropped: this frame's survivors whose refinement did not end OK (0 without refinement). */
SSBA_API int ssba_track_stream_push(ssba_track_stream *stream, const uint8_t *left, const uint8_t *right, const int16_t *disp16, uint32_t *track_id,
                                    double *uvd, uint32_t *num_observations, uint32_t *num_dropped);

/* The last `frames` pushed frames, 1 <= frames <= min(window, pushed frames), in ssba_frontend_vo's input format as
 * ssba_track_sequence writes it: state_start (frames + 1), point_id and uvd with room for `capacity` observations. */
SSBA_API int ssba_track_stream_window(ssba_track_stream *stream, uint32_t frames, uint64_t capacity, uint32_t *state_start, uint32_t *point_id,
                                      double *uvd, uint64_t *num_observations, uint32_t *num_points);

/* ---- odometry ----------------------------------------------------------------------------------------------------------- */
#define SSBA_TRACK_ODOMETRY_MAX 4096          /* matches and hypotheses */
#define SSBA_TRACK_ODOMETRY_MAX_REFINE 1024   /* refine_iterations */
#define SSBA_TRACK_POSE_OK 0
#define SSBA_TRACK_POSE_FIRST_FRAME 1
#define SSBA_TRACK_POSE_FEW_MATCHES 2
#define SSBA_TRACK_POSE_FEW_INLIERS 3
#define SSBA_TRACK_POSE_NUMERICAL 4

/* ssba_track_default_odometry_params: camera all zero (the caller sets it), ransac_iterations 400 and ransac_threshold 4.0 (the
 * reference's), refine_iterations 20 (0: the RANSAC pose is the answer), observation_variance 4.0 (node :246), first_pose the
 * identity */
typedef struct {
    ssba_camera camera;
    uint32_t ransac_iterations;
    double ransac_threshold;
    uint32_t refine_iterations;
    double observation_variance;
    double first_pose[12];
} ssba_track_odometry_params;
SSBA_API void ssba_track_default_odometry_params(ssba_track_odometry_params *params);

/* num_iterations counts the minimiser's iteration records, the initial one included (0: no refinement ran); the costs are those
 * of the refinement (0 when none ran) */
typedef struct {
    int32_t status;
    uint32_t num_matches, num_inliers, num_iterations;
    double initial_cost, final_cost;
} ssba_track_pose_info;

/* Only before the stream's first push (SSBA_ERR_STATE afterwards, and when it is enabled already).  Allocates everything the
 * odometry needs: a push still allocates nothing. */
SSBA_API int ssba_track_stream_enable_odometry(ssba_track_stream *stream, const ssba_track_odometry_params *params);

/* The result of the last push: no device work, the numbers came down in the push's one copy.  info may be NULL. */
SSBA_API int ssba_track_stream_pose(ssba_track_stream *stream, double T_k_km1[12], double T_k_0[12], ssba_track_pose_info *info);

/* The odometry's kernels on a list the caller supplies: n matches paired by position, uvd_prev and uvd_cur with 3 doubles each
 * (NULL allowed when n = 0), frame_index for the draws.  T_ransac (12), inlier (n flags), cost_log and step_ok
 * (refine_iterations + 1 entries each: the minimiser's records, NaN / 0 behind the last) may be NULL; T (12) and info not. */
SSBA_API int ssba_track_relative_pose(const ssba_track_odometry_params *params, uint32_t frame_index, uint32_t n, const double *uvd_prev,
                                      const double *uvd_cur, int device, double *T_ransac, uint8_t *inlier, double *T, ssba_track_pose_info *info,
                                      double *cost_log, int32_t *step_ok);

/* NULL is allowed.  Nothing else may use the stream while or after this runs. */
SSBA_API void ssba_track_stream_destroy(ssba_track_stream *stream);

SSBA_API const char *ssba_track_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SSBA_TRACKS_H_ */
