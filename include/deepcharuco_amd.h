/*
 * deepcharuco_amd.h -- C ABI of libdeepcharuco_amd.so (MI355X / gfx950 only).
 *
 * The reference (JunkyByte/deepcharuco) has no FFI: its boundary is the Python
 * function API of src/inference.py.  This header is what a binding for that
 * path links against; deepcharuco_amd/_lib.py binds it with ctypes and
 * deepcharuco_amd/inference.py rebuilds the reference's Python API on top
 * (see INTEGRATION.md).  Each entry point cites the reference interface it
 * replaces (paths relative to /root/reference/src).
 *
 * Conventions
 *   - every `d_` pointer is a DEVICE pointer owned by the caller (e.g. a
 *     torch tensor's data_ptr()); every `h_` pointer is host memory;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no
 *     entry point synchronises the device or allocates after create();
 *   - return value: 0 ok, <0 argument/shape error (DCX_E_*), >0 hipError_t;
 *   - no C++ exception crosses the boundary; handles are not thread-safe
 *     (use one handle per stream);
 *   - activations inside the library use the "C4" layout
 *     [N][C/4][H][W][4] float32 (channel-quad planar); NCHW only at the API.
 */
#ifndef DEEPCHARUCO_AMD_H
#define DEEPCHARUCO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCX_E_ARG      (-1)   /* null pointer / bad scalar */
#define DCX_E_SHAPE    (-2)   /* H or W below 8, patch not 24x24, capacity overflow ... */
#define DCX_E_WS       (-3)   /* workspace too small */
#define DCX_E_NIDS     (-4)   /* n_ids outside [1, 63] at create(); dust_bin outside [0, 255] at decode */

typedef struct dcx_detector dcx_detector;   /* dcModel  (models/net.py:9-99)        */
typedef struct dcx_refiner  dcx_refiner;    /* RefineNet (models/refinenet.py:9-115) */

const char* dcx_version(void);
/* human readable text for a return code (static storage) */
const char* dcx_error_string(int code);

/* ---- model lifetime: replaces load_models() inference.py:73-84 ----------------------
 * h_tensors: host float32 arrays in the order deepcharuco_amd.weights.state_dict_keys()
 * gives, i.e. for every conv in forward order: weight (OIHW), bias and -- where a
 * BatchNorm2d follows -- gamma, beta, running_mean, running_var.  The library packs the
 * weights into its MFMA operand layout, folds eval-mode BN (eps 1e-5) into a per-channel
 * (alpha, beta') pair exactly as ATen's CPU inference path does, and uploads them.
 * Detector: 12 convs / 10 BN = 64 tensors; RefineNet: 12 convs / 11 BN = 68 tensors.   */
int dcx_detector_create(dcx_detector** out, const float* const* h_tensors, int n_tensors, int n_ids);
int dcx_detector_destroy(dcx_detector* det);
int dcx_refiner_create(dcx_refiner** out, const float* const* h_tensors, int n_tensors);
int dcx_refiner_destroy(dcx_refiner* rf);

/* ---- workspace sizing (bytes of device scratch the forward calls need) -------------- */
size_t dcx_detector_workspace_bytes(const dcx_detector* det, int batch, int height, int width);
size_t dcx_refiner_workspace_bytes(const dcx_refiner* rf, int max_patches);

/* ---- colour conversion: cv2.cvtColor(img, cv2.COLOR_BGR2GRAY) call at inference.py:40 ---------
 * 8-bit BGR frames (interleaved, row pitch / frame stride in BYTES) -> dense gray u8 [B][H][W].  OpenCV is third-party and not
 * vendored in the reference ("parity unpinned" for this one step); the reference pins opencv-contrib-python
 * >= 4.6, < 4.12 (requirements.txt:5).
 *   dcx_bgr2gray           OpenCV 4.x RGB2Gray<uchar> (imgproc/src/color.hpp: gray_shift = 15, BY15 / GY15 / RY15):
 *                              gray = (3735 B + 19235 G + 9798 R + 16384) >> 15
 *   dcx_bgr2gray_legacy14  the older 14-bit form (B2Y / G2Y / R2Y, yuv_shift; in 4.x only 16-bit images and YUV use it):
 *                              gray = (1868 B + 9617 G + 4899 R + 8192) >> 14
 * The two differ by one level on ~0.26 % of colour pixels and never on gray-replicated input.                          */
int dcx_bgr2gray(const uint8_t* d_bgr, long frame_stride, int pitch, int batch, int height, int width,
                 uint8_t* d_gray, void* stream);
int dcx_bgr2gray_legacy14(const uint8_t* d_bgr, long frame_stride, int pitch, int batch, int height, int width,
                          uint8_t* d_gray, void* stream);

/* ---- pre-processing ------------------------------------------------------------------
 * pre_bgr_image models/model_utils.py:46-50:  out = (float(g) - 128) / 255 (IEEE division).
 * d_gray [n] u8 -> d_out [n] f32.                                                        */
int dcx_pre_image(const uint8_t* d_gray, float* d_out, size_t n, void* stream);

/* ---- detector forward: dcModel.forward net.py:50-80 / infer_image net.py:82-99 -------
 * Input either u8 gray frames (d_frames_u8, row pitch in bytes, frame stride in bytes;
 * normalised on the fly exactly like dcx_pre_image) or already-normalised f32 images
 * (d_images_f32, dense [B][H][W]); exactly one of the two must be non-null.
 * Outputs (either may be null): logits in NCHW, loc [B][65][H/8][W/8], ids [B][n_ids+1][H/8][W/8].
 * The C4 logits stay in the workspace for dcx_detector_decode().                          */
int dcx_detector_forward(const dcx_detector* det,
                         const uint8_t* d_frames_u8, long frame_stride, int pitch,
                         const float* d_images_f32,
                         int batch, int height, int width,
                         void* d_ws, size_t ws_bytes,
                         float* d_loc_nchw, float* d_ids_nchw, void* stream);

/* ---- decode: pred_to_keypoints model_utils.py:81-88 (= pred_argmax :53-78 +
 *      label_to_keypoints :91-124), batched -----------------------------------------------
 * Per cell: loc = argmax_c loc_logits (first max), id = argmax_c ids_logits, id = dust_bin
 * where loc == 64; cells with id != dust_bin emit a row {x = 8*cx + loc%8, y = 8*cy + loc/8,
 * id, cell = cy*Wc + cx} in raster order per frame.  d_counts[b] = number of firing cells
 * (may exceed kmax; only the first kmax rows are stored).  d_rows: int32 [B][kmax][4].
 * dust_bin is the reference's `dust_bin_ids` argument: any value in [0, 255] (else DCX_E_NIDS) with the reference's
 * semantics `ids != dust_bin_ids` -- it normally equals n_ids but is not required to.
 * Optional dense maps d_loc_argmax / d_ids_argmax: int32 [B][Hc][Wc] (ids map is post-mask).
 * Truncation: d_counts[b] is never capped; d_rows[b][k] is written for k < min(d_counts[b], kmax) and left untouched beyond
 * (a frame that fires nothing writes no row); kmax <= 0 is DCX_E_SHAPE.
 * Non-finite logits: the arg-max follows torch.argmax -- NaN counts as the maximum and the first NaN wins, else the first
 * largest value (+inf and -inf order like any number; all -inf gives class 0).  That holds for the three entries below, which
 * take or re-read logits a caller can see.  The fused pipeline (dcx_infer_batch) never stores its logits and only non-finite
 * WEIGHTS could make them non-finite: its arg-max on such logits is unspecified.
 * dcx_detector_decode reads the logits the preceding dcx_detector_forward left in d_ws and
 * uses 4 bytes per cell of scratch in it (arg-max of all cells in parallel, then one ordered
 * compaction per frame); dcx_pred_to_keypoints takes caller NCHW logits (the reference's own
 * signature) and needs no scratch (one workgroup per frame).                                */
int dcx_detector_decode(const dcx_detector* det, int batch, int height, int width,
                        void* d_ws, int dust_bin, int kmax,
                        int32_t* d_counts, int32_t* d_rows,
                        int32_t* d_loc_argmax, int32_t* d_ids_argmax, void* stream);
int dcx_pred_to_keypoints(const float* d_loc_nchw, const float* d_ids_nchw,
                          int batch, int n_loc, int n_ids1, int hc, int wc,
                          int dust_bin, int kmax,
                          int32_t* d_counts, int32_t* d_rows,
                          int32_t* d_loc_argmax, int32_t* d_ids_argmax, void* stream);
/* label_to_keypoints model_utils.py:91-124 on caller label maps (class indices, int64 [B][Hc][Wc], as pred_argmax returns them):
 * mask = ids != dust_bin, x = 8*ix + loc%8, y = 8*iy + loc/8, rows in torch.nonzero's raster order -- the second half of
 * dcx_pred_to_keypoints as its own entry, like in the reference.  d_codes: 4 bytes per cell of scratch; d_bad (nullable int32):
 * set to 1 when a label lies outside [0, 255].  A dust_bin outside [0, 255] equals no label: every cell fires.                                                                            */
int dcx_label_to_keypoints(const long long* d_loc, const long long* d_ids, int batch, int hc, int wc, int dust_bin, int kmax,
                           int32_t* d_counts, int32_t* d_rows, int32_t* d_codes, int32_t* d_bad, void* stream);

/* ---- patch table: compacts the per-frame rows of a batch into one patch list ----------
 * d_table int32 [B*kmax][4] = {frame, x, y, slot = frame*kmax + k}; d_total int32 [1] =
 * sum_b min(counts[b], kmax).  Device-side replacement for the host syncs at
 * model_utils.py:114 / inference.py:51.  Frames in order, each frame's rows in order, no gaps: frame b's entries start at
 * sum_{a<b} min(counts[a], kmax); counts above kmax are capped (the rows beyond were never stored), frames at 0 take no entry.
 * Entries at and beyond *d_total are left untouched.  Any batch >= 1 (one workgroup walks the frames 256 at a time).        */
int dcx_build_patch_table(const int32_t* d_counts, const int32_t* d_rows, int batch, int kmax,
                          int32_t* d_table, int32_t* d_total, void* stream);

/* ---- extract_patches models/model_utils.py:19-36 ---------------------------------------
 * patch[p][i][j] = img[y-12+i][x-12+j], 0.0f outside the image (zero pad of the NORMALISED
 * image).  d_table rows {frame,x,y,slot}; patches beyond *d_total (if non-null) are skipped:
 * d_patches[p] is left untouched for p >= *d_total.  With d_total == NULL all max_patches table rows are read.
 * u8 variant normalises on the fly ((float(g) - 128) / 255, as dcx_pre_image); frames are windows of a caller buffer: frame f's
 * pixel (y, x) is the byte d_frames[f*frame_stride + y*pitch + x], bytes outside a window are never read.
 * f32 variant takes dense normalised images [B][H][W].  Any height, width >= 1 (a frame may be smaller than a patch).
 * The table is trusted: frame indices must lie inside the frames passed, *d_total <= max_patches.                      */
int dcx_extract_patches_u8(const uint8_t* d_frames, long frame_stride, int pitch, int height, int width,
                           const int32_t* d_table, const int32_t* d_total, int max_patches,
                           float* d_patches, void* stream);
int dcx_extract_patches_f32(const float* d_images, int height, int width,
                            const int32_t* d_table, const int32_t* d_total, int max_patches,
                            float* d_patches, void* stream);

/* ---- RefineNet: forward refinenet.py:49-83 + infer_patches :85-115 ---------------------
 * d_patches f32 [P][24][24] -> per patch flat argmax (first max) of the 64x64 heat-map:
 * d_corners int32 [P][2] = {col,row}; if d_table/d_xy given, d_xy[slot] = {(col-32)/8 + x,
 * (row-32)/8 + y} (float32, refinenet.py:114).  d_heat (nullable) f32 [P][64][64] receives
 * the raw heat-map.  Patches >= *d_total (if non-null) are skipped: their d_corners / d_heat entries and every d_xy slot no
 * live table row names are left untouched.  The slots are the table's (frame*kmax + k from dcx_build_patch_table), so d_xy
 * must hold the largest slot + 1 pairs; *d_total <= max_patches is trusted.  Skipped patches are skipped in every layer: the
 * call writes at most dcx_refiner_workspace_bytes(rf, *d_total) bytes of d_ws (none when *d_total is 0).                  */
int dcx_refiner_forward(const dcx_refiner* rf, const float* d_patches, int max_patches,
                        const int32_t* d_total, const int32_t* d_table,
                        void* d_ws, size_t ws_bytes,
                        int32_t* d_corners, float* d_xy, float* d_heat, void* stream);

/* ---- speedy_bargmax2d models/model_utils.py:39-43 --------------------------------------
 * d_x f32 [K][h][w] -> d_out int32 [K][2] = {col,row} of the first maximum (torch.max: a NaN is the maximum, the first one wins). */
int dcx_argmax2d(const float* d_x, int k, int h, int w, int32_t* d_out, void* stream);

/* ---- whole path for a batch: infer_image inference.py:32-70 without host syncs ----------
 * frames u8 -> detector -> per-cell arg-max + dust-bin rule -> ordered compaction -> RefineNet on every firing cell -> xy.
 *
 * Frames: DCX_PIX_GRAY8 (what inference.py:40 produces) or interleaved BGR (what infer_image is handed, inference.py:32; the
 * conversion of dcx_bgr2gray / dcx_bgr2gray_legacy14 happens in the first layer's load, the gray frame is never stored);
 * frame_stride and pitch in BYTES.
 *
 * Results -- the batch's CORNER POOL.  The reference refines every firing cell of a frame (inference.py:51-57, no cap), so
 * there is no per-frame capacity: frame b's corners occupy the pool slots [d_starts[b], d_starts[b] + d_counts[b]) in raster
 * order (torch.nonzero's, model_utils.py:112), whatever their number, as long as the BATCH fits: sum_b counts[b] <= pool.
 *   d_counts int32 [B]        firing cells of frame b (never truncated)
 *   d_starts int32 [B]        first pool slot of frame b; which frame comes first in the pool is unspecified
 *   d_rows   int32 [pool][4]  (x, y, id, cell = cy*Wc + cx)
 *   d_xy     f32   [pool][2]  RefineNet's corners_og (refinenet.py:114); required iff rf != NULL
 *   d_conf   f32   [pool][2]  nullable: soft-max probability of the winning loc class (65-way) and ids class (n_ids+1-way) of
 *                             the cell -- the "confidences" the docstring of pred_to_keypoints (model_utils.py:81-84) mentions;
 *                             the reference never thresholds on them and neither does this library
 * Slots >= pool are dropped: when sum(counts) > pool the caller re-runs with a larger pool (complete frames are still valid).
 * d_ws must hold dcx_pipeline_workspace_bytes().  rf may be null (detector + decode only).
 *
 * WORKSPACES, here and for every entry that takes a d_ws, d_workspace or d_front: the contents of a workspace at entry do not
 * matter; the call writes nothing outside [d_ws, d_ws + *_workspace_bytes()) and its output buffers.  A workspace may hold
 * zeros, NaN bit patterns or what any earlier call left in it, of another batch size or shape; nothing has to be cleared between
 * calls (tests/test_gpu_workspace_contract.py holds every entry to this on poisoned, exact-size buffers between guards).   */
#define DCX_PIX_GRAY8          0
#define DCX_PIX_BGR8           1   /* OpenCV 4.x 15-bit constants, = dcx_bgr2gray          */
#define DCX_PIX_BGR8_LEGACY14  2   /* 14-bit constants,            = dcx_bgr2gray_legacy14 */
size_t dcx_pipeline_workspace_bytes(const dcx_detector* det, const dcx_refiner* rf,
                                    int batch, int height, int width, int pool);
int dcx_infer_batch(const dcx_detector* det, const dcx_refiner* rf,
                    const uint8_t* d_frames_u8, long frame_stride, int pitch, int pixel_format,
                    int batch, int height, int width, int dust_bin, int pool,
                    void* d_ws, size_t ws_bytes,
                    int32_t* d_counts, int32_t* d_starts, int32_t* d_rows, float* d_xy, float* d_conf, void* stream);
/* The same path in two calls, for a caller that runs the NEXT batch's first layer beside the current batch's convolutions:
 * dcx_detector_front runs the detector's conv1a (u8 load, BN, ReLU) of a batch into a PREFETCH SET -- conv1a's output,
 * batch x 64 x H x W f32, and the control words of the batch (pool cursor, frame tickets), which it clears -- on the stream it is
 * given; it depends on nothing but the frames.  dcx_infer_batch_prefetched then does what dcx_infer_batch does from conv1b on:
 * it reads the set instead of launching conv1a and leaves the same results, bit for bit.  The set is in use from the front
 * call until the prefetched call's last kernel has finished (RefineNet reads the cursor as its patch count): two sets let
 * consecutive batches alternate.  Order the two calls with an event if they are on different streams; frames, shape and pixel
 * format must be the same in both.  detector_done_event (a hipEvent_t, nullable) is recorded on the stream behind the detector's last
 * convolution launch: the point from which the launches are small until RefineNet's conv1b -- where a front for the next batch
 * does least harm.  d_front must hold dcx_front_bytes() (0: bad arguments); DCX_E_WS if it does not.          */
size_t dcx_front_bytes(const dcx_detector* det, int batch, int height, int width);
int dcx_detector_front(const dcx_detector* det, const uint8_t* d_frames_u8, long frame_stride, int pitch, int pixel_format,
                       int batch, int height, int width, void* d_front, size_t front_bytes, void* stream);
int dcx_infer_batch_prefetched(const dcx_detector* det, const dcx_refiner* rf,
                               const uint8_t* d_frames_u8, long frame_stride, int pitch, int pixel_format,
                               int batch, int height, int width, int dust_bin, int pool,
                               void* d_ws, size_t ws_bytes, void* d_front, size_t front_bytes,
                               int32_t* d_counts, int32_t* d_starts, int32_t* d_rows, float* d_xy, float* d_conf,
                               void* detector_done_event, void* stream);
/* hipStreamSynchronize(stream) -> the hipError_t.  Waits in the HIP runtime this library was linked against, which is the one
 * whose streams the caller passes here (torch's, in the Python package): a second copy of the runtime loaded beside it would not
 * know those streams, and its synchronisation of the default stream would return without waiting.                           */
int dcx_stream_synchronize(void* stream);

/* ---- solve_pnp inference.py:15-29 (cv2.solvePnP, default flags = SOLVEPNP_ITERATIVE) on the device, per frame of a pool --
 * Reads a corner pool in place, in the layout dcx_infer_batch writes (or a caller-built one: counts / starts + the id column of
 * rows + xy): frame b's points are the slots [d_starts[b], d_starts[b] + d_counts[b]); object point of id i =
 * ((1 + i % (row_count-1)) * square_len, (1 + i / (row_count-1)) * square_len, 0) rounded to float32 like the reference's
 * np.float32 table (inference.py:20-26; square_len is a double so that the rounding matches); image point = d_xy (RefineNet's
 * corners) or, with d_xy == NULL, the integer x, y of d_rows (inference.py:27).  All arithmetic fp64: undistortPoints (5 rounds),
 * planar DLT homography + OpenCV's decomposition, Levenberg-Marquardt on the pixel reprojection error (<= 20 steps, stop at
 * |dp|/|p| < FLT_EPSILON); deepcharuco_amd/pnp.py restates the steps (solve_pnp_host).  One wavefront per frame, grid = batch.
 * h_camera9: K row major, K[0][1] must be 0 (DCX_E_ARG otherwise); h_dist: n_dist = 0, 4, 5 or 8 OpenCV coefficients
 * (12 / 14 -> DCX_E_ARG).  Both are copied into the kernel arguments at the call (a captured hipGraph keeps them).
 * d_status int32 [B]: DCX_PNP_*.  d_pose f64 [B][8] = rvec(3), tvec(3), rms reprojection error (px), accepted LM steps; zeros
 * unless DCX_PNP_OK.  Unlike cv2.solvePnP, collinear points, a rank-deficient homography, a point behind the camera or a
 * non-finite result give DCX_PNP_DEGENERATE / DCX_PNP_NONFINITE instead of a pose.                                        */
#define DCX_PNP_OK          0
#define DCX_PNP_TOO_FEW     1   /* fewer than 4 points (inference.py:16-17) */
#define DCX_PNP_TRUNCATED   2   /* starts[b] + counts[b] > pool: the frame's corners did not all fit the pool */
#define DCX_PNP_BAD_ID      3   /* an id outside [0, (col_count-1)*(row_count-1)): the reference raises IndexError */
#define DCX_PNP_DEGENERATE  4
#define DCX_PNP_NONFINITE   5
int dcx_solve_pnp_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows,
                       const float* d_xy /* NULL = use integer rows x,y */, int batch, int pool,
                       int col_count, int row_count, double square_len,
                       const double* h_camera9, const double* h_dist, int n_dist,
                       int32_t* d_status, double* d_pose /* [B][8] = rvec3, tvec3, rms_px, iterations */,
                       void* stream);

/* ---- the same solver behind a consensus search (cv2.solvePnPRansac's role): poses that survive mislabelled corners ---------
 * Pool, object points, image points, camera arguments and the per-frame checks (TOO_FEW, TRUNCATED, BAD_ID) as for
 * dcx_solve_pnp_pool; the frames' slot ranges must not overlap (each frame's inlier list lives at its own slots of the workspace).
 * Per frame, `iterations` hypotheses (1..4096), all of them evaluated (no confidence-based early exit: the work is fixed):
 * hypothesis h draws four rows (slots of the frame as the pool holds them, whatever their order) by a 32-bit counter hash of
 * (seed, counts[b], h, draw) -- not of b, so a frame gives the same
 * result wherever it stands in a batch -- with distinct ids and no three board points on a line (8 draws at most), takes the
 * planar pose through them (closed-form homography, OpenCV's decomposition, no LM) and scores the rows whose reprojection error
 * through the full distortion model is <= reproj_error px (finite, > 0); a row behind the camera is an outlier.  The winner is the
 * highest score, the lowest h among equals.  No hypothesis: DCX_PNP_DEGENERATE.  Fewer than max(min_inliers, 4) inliers:
 * DCX_PNP_NO_CONSENSUS.  Else d_pose[b] is dcx_solve_pnp_pool's solve over the winner's inlier rows alone (rms over them) and its
 * status the frame's.  deepcharuco_amd/pnp.py restates the steps (solve_pnp_ransac_host_full).
 * d_info int32 [B][2]: inlier count (the population of the frame's mask), winning hypothesis (-1: none).  d_inliers uint8 [pool]
 * (may be NULL): 1 at the winner's inlier slots (not recomputed after the refit, as in cv2); 0 at every slot of a frame that ends
 * without a pose; slots of no frame are not written.  d_workspace: dcx_solve_pnp_ransac_workspace_bytes(batch, pool, iterations)
 * bytes, 8-byte aligned (DCX_E_ARG if smaller).  Two launches on `stream`; no allocation, no synchronisation, no atomics: two
 * calls give the same bits and the call can be captured in a hipGraph.                                                       */
#define DCX_PNP_NO_CONSENSUS 6
size_t dcx_solve_pnp_ransac_workspace_bytes(int batch, int pool, int iterations);   /* 0 for refused arguments */
int dcx_solve_pnp_ransac_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows,
                              const float* d_xy /* NULL = use integer rows x,y */, int batch, int pool,
                              int col_count, int row_count, double square_len,
                              const double* h_camera9, const double* h_dist, int n_dist,
                              int iterations, double reproj_error, int min_inliers, unsigned seed,
                              void* d_workspace, size_t workspace_bytes,
                              int32_t* d_status, double* d_pose /* [B][8] */, int32_t* d_info /* [B][2] */,
                              uint8_t* d_inliers /* [pool], may be NULL */, void* stream);

/* ---- camera calibration from the views of a ChArUco board in a pool (cv2.calibrateCamera with default flags, planar target; ----
 * ---- its flags and the rational model: dcx_calibrate_flags_pool below) -------------------------------------------------------
 * The camera model solve_pnp needs (calib_intrinsics.py:44, cv2.calibrateCamera) from the corners of
 * `batch` views, read in place from a corner pool laid out as for dcx_solve_pnp_pool (same object points, same image points, same
 * per-view checks and DCX_PNP_* codes in d_view_status).  All fp64: OpenCV's initIntrinsicParams2D (principal point at
 * ((w-1)/2, (h-1)/2), per-view DLT homography, least squares for fx, fy), every view's pose by the PnP solver with that K and no
 * distortion, then joint Levenberg-Marquardt over fx, fy, cx, cy, k1, k2, p1, p2, k3 (skew 0) and every used view's pose (<= 30
 * accepted steps, stop at |dp|/|p| < DBL_EPSILON), each step by block elimination of the views' 6x6 pose blocks;
 * deepcharuco_amd/calib.py restates the steps (calibrate_camera_host_full).  A view that fails its checks is left out and reported.
 * UNLIKE every other entry point, this one SYNCHRONISES `stream`: the LM loop runs on the host and reads a state word from the
 * device after every attempt (their number depends on the data), so the call cannot be captured in a graph.
 * d_workspace: dcx_calibrate_workspace_bytes(batch) bytes of device memory (DCX_E_WS if smaller); nothing is allocated.
 * d_pose f64 [B][8] = rvec(3), tvec(3), the view's rms reprojection error at the solution (px), its point count (counts[b]);
 * every view gets its point count, the other words are zero unless the view was used and the calibration succeeded.
 * h_result f64 [16] = fx, fy, cx, cy, k1, k2, p1, p2, k3, rms (sqrt(sum |r|^2 / points used), cv2's return value), accepted LM
 * steps, attempts, views used, points used, DCX_CALIB_* status, 0; the first ten are zero unless DCX_CALIB_OK.
 * No atomics: two calls on the same input give the same bits.                                                               */
#define DCX_CALIB_OK          0
#define DCX_CALIB_NO_VIEWS    1   /* no view passed its checks */
#define DCX_CALIB_DEGENERATE  2   /* the init's 2x2 system or a damped step is singular, or the cost is not finite */
#define DCX_CALIB_NONFINITE   3
size_t dcx_calibrate_workspace_bytes(int batch);
int dcx_calibrate_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows,
                       const float* d_xy /* NULL = use integer rows x,y */, int batch, int pool,
                       int col_count, int row_count, double square_len, int image_width, int image_height,
                       void* d_workspace, size_t workspace_bytes,
                       int32_t* d_view_status /* [B] DCX_PNP_* */, double* d_pose /* [B][8] */,
                       double* h_result /* [16] */, void* stream);

/* ---- the same calibration with cv2.calibrateCamera's flags and the rational model ----------------------------------------------
 * dcx_calibrate_pool's pool, per-view checks, DCX_PNP_* / DCX_CALIB_* codes, d_view_status and d_pose; `flags` are cv2's values
 * below, any other bit is DCX_E_ARG (thin prism, tilted, FIX_S*, FIX_TANGENT_DIST, USE_LU / USE_QR).  The parameter vector is always
 * theta12 = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6, and the flags say which entries the solve moves
 * (deepcharuco_amd/calib.py restates every rule: calibrate_camera_host_full with flags).  Steps:
 * 1. start.  Without USE_INTRINSIC_GUESS: dcx_calibrate_pool's (Zhang's focal lengths, the image centre, zero distortion); with
 *    FIX_ASPECT_RATIO OpenCV's rule on it, a = h_camera9[0] / h_camera9[4], tf = (fx + fy) / (a + 1), fx = a tf, fy = tf.  With the
 *    guess: theta12 = h_camera9 and h_dist (n_dist = 0, 4, 5 or 8, missing coefficients 0; h_dist must be NULL and n_dist 0 without
 *    the guess), and the per-view checks of the default start without its init rows.  h_camera9 is required by either flag.
 * 2. every view's pose by the PnP solver through the start model, distortion included.
 * 3. dcx_calibrate_pool's joint Levenberg-Marquardt (same damping, caps and stop rule, |dp| / |p| over all parameters) in which
 *    FIX_PRINCIPAL_POINT fixes cx cy, FIX_FOCAL_LENGTH fx fy, ZERO_TANGENT_DIST sets p1 = p2 = 0 and fixes them, FIX_Ki fixes ki at its
 *    start value, k4 k5 k6 stay at their start values without RATIONAL_MODEL, and FIX_ASPECT_RATIO ties fx = a fy (fy moves, every
 *    trial step writes fx = a * fy, one multiplication).  A fixed parameter comes back with the bits it started with.  The flags
 *    are a linear map on the intrinsic columns that commutes with the block elimination, so only the reduced solve knows them.
 *    While k4 k5 k6 are zero and fixed the 9-parameter kernels of dcx_calibrate_pool run; with RATIONAL_MODEL, or a guess whose
 *    k4 k5 k6 are not all zero, the 12-parameter model's.
 * d_workspace: dcx_calibrate_flags_workspace_bytes(batch, flags) bytes (0 for refused arguments; DCX_E_WS if smaller); a guess
 * with non-zero k4 k5 k6 needs the size of flags | DCX_CALIB_RATIONAL_MODEL.  h_result f64 [20] = theta12, rms, accepted LM steps,
 * attempts, views used, points used, DCX_CALIB_* status, 0, 0; the first 13 are zero unless DCX_CALIB_OK.  SYNCHRONISES `stream`
 * like dcx_calibrate_pool; no atomics: two calls give the same bits; nothing is allocated.  Rational models are to be compared by
 * where they project, not coefficient by coefficient.                                                                          */
#define DCX_CALIB_USE_INTRINSIC_GUESS  0x0001
#define DCX_CALIB_FIX_ASPECT_RATIO     0x0002
#define DCX_CALIB_FIX_PRINCIPAL_POINT  0x0004
#define DCX_CALIB_ZERO_TANGENT_DIST    0x0008
#define DCX_CALIB_FIX_FOCAL_LENGTH     0x0010
#define DCX_CALIB_FIX_K1               0x0020
#define DCX_CALIB_FIX_K2               0x0040
#define DCX_CALIB_FIX_K3               0x0080
#define DCX_CALIB_FIX_K4               0x0800
#define DCX_CALIB_FIX_K5               0x1000
#define DCX_CALIB_FIX_K6               0x2000
#define DCX_CALIB_RATIONAL_MODEL       0x4000
size_t dcx_calibrate_flags_workspace_bytes(int batch, int flags);
int dcx_calibrate_flags_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows,
                             const float* d_xy /* NULL = use integer rows x,y */, int batch, int pool,
                             int col_count, int row_count, double square_len, int image_width, int image_height,
                             int flags, const double* h_camera9 /* NULL without a guess or ratio */,
                             const double* h_dist, int n_dist,
                             void* d_workspace, size_t workspace_bytes,
                             int32_t* d_view_status /* [B] DCX_PNP_* */, double* d_pose /* [B][8] */,
                             double* h_result /* [20] */, void* stream);

/* ---- the same calibration behind a consensus search: a camera model that survives mislabelled corners -----------------------
 * Pool, object points, image points and the per-view checks as for dcx_calibrate_pool; the views' slot ranges must not overlap
 * (DCX_E_ARG, looked for on the device before anything is written: each view's surviving rows live at its own slots of the
 * workspace).  Steps, restated in deepcharuco_amd/calib.py (calibrate_camera_ransac_host_full):
 * B. per view, `iterations` hypotheses (1..4096) drawn by dcx_solve_pnp_ransac_pool's sampler, all evaluated: the closed-form
 *    homography through the four rows maps board xy to RAW pixels (no camera model exists yet, so nothing is undistorted and no
 *    pose can be scored), and the score is the rows whose transfer error is <= consensus_error px (finite, > 0; a row with
 *    q_z <= 0 is an outlier).  The winner is the highest score, the lowest h among equals.  No hypothesis: DCX_PNP_DEGENERATE;
 *    fewer than max(min_inliers, 4) inliers: DCX_PNP_NO_CONSENSUS; either way the view is left out.
 * C. dcx_calibrate_pool, unchanged, over the surviving rows of the views that still stand.
 * D. at most `rounds` (0..8) times: every row of every view the solve used is projected through the solved model and pose; the
 *    new mask is error <= reproj_error px (finite, > 0); a view left with fewer than max(min_inliers, 4) rows becomes
 *    DCX_PNP_NO_CONSENSUS; excluded views never come back.  If no mask changed the result is stable; else C runs again from
 *    scratch on the new masks.  The outputs are always those of the last solve and the masks it was given.
 * d_view_status, d_pose, h_result as dcx_calibrate_pool, except: the status of a view left out by B or D is that step's,
 * d_pose[b][6] and h_result[9], [13] are over inlier rows, d_pose[b][7] is the rows OFFERED (counts[b]), and h_result[15] =
 * solves + 16 * stable.  d_info int32 [B][2]: the view's inlier count, its winning hypothesis (-1: none).  d_inliers uint8 [pool]
 * (may be NULL): the mask the last solve was given, 0 at every slot of a view that was left out; slots of no view are not
 * written.  d_workspace: dcx_calibrate_ransac_workspace_bytes(batch, pool, iterations) bytes, 8-byte aligned (DCX_E_WS if
 * smaller); nothing is allocated.  Like dcx_calibrate_pool this entry point SYNCHRONISES `stream` (once for the overlap word, in
 * every solve, and once per round for the "changed" word) and cannot be captured in a graph.  No atomics: two calls give the
 * same bits.                                                                                                                 */
size_t dcx_calibrate_ransac_workspace_bytes(int batch, int pool, int iterations);   /* 0 for refused arguments */
int dcx_calibrate_ransac_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows,
                              const float* d_xy /* NULL = use integer rows x,y */, int batch, int pool,
                              int col_count, int row_count, double square_len, int image_width, int image_height,
                              int iterations, double consensus_error, double reproj_error, int min_inliers, int rounds,
                              unsigned seed, void* d_workspace, size_t workspace_bytes,
                              int32_t* d_view_status /* [B] DCX_PNP_* */, double* d_pose /* [B][8] */,
                              int32_t* d_info /* [B][2]: inliers, winner */, uint8_t* d_inliers /* [pool], may be NULL */,
                              double* h_result /* [16] */, void* stream);

/* ---- stereo extrinsic calibration from two corner pools (cv2.stereoCalibrate with CALIB_FIX_INTRINSIC, planar target) ---------
 * Two rigidly mounted cameras 0 and 1 with known models (h_camera9_c, h_dist_c, n_dist_c as for dcx_solve_pnp_pool; they may
 * differ) and one corner pool each, laid out as for dcx_solve_pnp_pool, with the same `batch`: frame t of pool 0 and frame t of
 * pool 1 show the same board at the same instant.  The two views of a timestamp need no common id.  Result: the rig transform
 * (R, T) in cv2's convention, q1 = R q0 + T, and the board's pose P_t in camera 0's frame for every timestamp used.  All fp64;
 * deepcharuco_amd/stereo.py restates the steps (stereo_calibrate_host_full):
 * 1. per view, d_mask_c (uint8 by SLOT of pool c, the format of the d_inliers that dcx_solve_pnp_ransac_pool and
 *    dcx_calibrate_ransac_pool write; NULL keeps every row) drops the rows with 0; then the checks of dcx_solve_pnp_pool, on
 *    the rows kept: fewer than 4 DCX_PNP_TOO_FEW, a frame cut by the pool DCX_PNP_TRUNCATED, an id outside the board
 *    DCX_PNP_BAD_ID.  With a mask the slot ranges of that pool's frames must not overlap (DCX_E_ARG, found on the device: a
 *    frame's kept rows are listed at its own slots of the workspace; the outputs are then unspecified).
 * 2. per view, dcx_solve_pnp_pool's solve with that camera's model (a failure: DCX_PNP_DEGENERATE / DCX_PNP_NONFINITE).  A
 *    timestamp is a pair, and is used, only if both of its views are DCX_PNP_OK.
 * 3. rig init: per pair R_t = R1_t R0_t^T, T_t = t1_t - R_t t0_t; the element-wise LOWER median over the pairs (element
 *    (n - 1) / 2 of the sorted values) of the 9 + 3 entries, the median matrix orthonormalised by its polar factor, then
 *    Rodrigues.  (cv2 takes the median of rotation vectors, which wrap near pi.)  P_t starts at camera 0's own pose.
 * 4. joint Levenberg-Marquardt over (rvec(R), T) and every pair's P_t on the pixel reprojection error of both cameras, the rules
 *    of dcx_calibrate_pool (<= 30 accepted steps, stop at |dp|/|p| < DBL_EPSILON where cv2's default criteria use 1e-6), each
 *    step by block elimination of the pairs' 6x6 pose blocks and a 6x6 Cholesky.
 * Like dcx_calibrate_pool this entry point SYNCHRONISES `stream`: once for the rig init (the pairs' R_t, T_t are copied to the
 * host, where the medians are taken) and after every LM attempt (a state word; their number depends on the data), so the call
 * cannot be captured in a graph.  d_workspace: dcx_stereo_calibrate_workspace_bytes(batch, pool0, pool1) bytes of device
 * memory, 8-byte aligned (DCX_E_WS if smaller); no device memory is allocated.
 * d_view_status int32 [B][2]: DCX_PNP_* of view (t, camera).  d_pose f64 [B][8] = P_t as rvec(3), tvec(3), the pair's rms
 * reprojection error over both views (px), the rows of both views; all zero unless the pair was used and the status is
 * DCX_STEREO_OK.  d_view_info f64 [B][2][2] = per view its rms at the solution (zero unless its pair was used and the status is
 * DCX_STEREO_OK) and the rows it brings after its mask (every view; 0 for a frame that is empty or cut by the pool).
 * h_result f64 [16] = rvec(R) (3), T (3), rms (sqrt(sum |r|^2 / points used) over both cameras, cv2's return value), accepted
 * LM steps, attempts, pairs used, points used (the pairs found and their rows, whatever the status), DCX_STEREO_* status, 0...;
 * the first seven are zero unless DCX_STEREO_OK.
 * No atomics: two calls on the same input give the same bits.                                                               */
#define DCX_STEREO_OK          0
#define DCX_STEREO_NO_PAIRS    1   /* no timestamp has two usable views */
#define DCX_STEREO_DEGENERATE  2   /* the median matrix or a damped step is singular, or the cost is not finite */
#define DCX_STEREO_NONFINITE   3
size_t dcx_stereo_calibrate_workspace_bytes(int batch, int pool0, int pool1);   /* 0 for refused arguments */
int dcx_stereo_calibrate_pool(const int32_t* d_counts0, const int32_t* d_starts0, const int32_t* d_rows0,
                              const float* d_xy0 /* NULL = use integer rows x,y */, const uint8_t* d_mask0 /* [pool0] or NULL */,
                              const int32_t* d_counts1, const int32_t* d_starts1, const int32_t* d_rows1,
                              const float* d_xy1, const uint8_t* d_mask1 /* [pool1] or NULL */,
                              int batch, int pool0, int pool1, int col_count, int row_count, double square_len,
                              const double* h_camera9_0, const double* h_dist0, int n_dist0,
                              const double* h_camera9_1, const double* h_dist1, int n_dist1,
                              void* d_workspace, size_t workspace_bytes,
                              int32_t* d_view_status /* [B][2] DCX_PNP_* */, double* d_pose /* [B][8] */,
                              double* d_view_info /* [B][2][2] */, double* h_result /* [16] */, void* stream);

/* dcx_stereo_calibrate_pool over a pair whose cameras need not be pinholes: model0, model1 are DCX_CAMERA_*.  A
 * DCX_CAMERA_FISHEYE camera is the model of the dcx_fisheye_* entries: its h_dist holds k1..k4 with n_dist = 4, or n_dist = 0 for
 * zeros; its views are solved by dcx_fisheye_solve_pnp_pool's solver (a view with a pixel outside the model is
 * DCX_PNP_DEGENERATE) and its rows enter the joint solve through that model's projection.  Everything else (steps, outputs,
 * statuses, h_result, synchronisation, the bits' repeatability) is dcx_stereo_calibrate_pool's, and
 * dcx_stereo_calibrate_workspace_bytes serves this entry too: the workspace layout does not depend on the models.  With both
 * models DCX_CAMERA_PINHOLE the call IS dcx_stereo_calibrate_pool: the same kernels, the same bits.  DCX_E_ARG also for a model
 * other than these two and for a fisheye camera with n_dist of 5 or 8.                                                          */
#define DCX_CAMERA_PINHOLE 0
#define DCX_CAMERA_FISHEYE 1
int dcx_stereo_calibrate_models_pool(const int32_t* d_counts0, const int32_t* d_starts0, const int32_t* d_rows0, const float* d_xy0,
                                     const uint8_t* d_mask0, const int32_t* d_counts1, const int32_t* d_starts1,
                                     const int32_t* d_rows1, const float* d_xy1, const uint8_t* d_mask1, int batch, int pool0,
                                     int pool1, int col_count, int row_count, double square_len, const double* h_camera9_0,
                                     const double* h_dist0, int n_dist0, const double* h_camera9_1, const double* h_dist1,
                                     int n_dist1, int model0, int model1, void* d_workspace, size_t workspace_bytes,
                                     int32_t* d_view_status /* [B][2] */, double* d_pose /* [B][8] */,
                                     double* d_view_info /* [B][2][2] */, double* h_result /* [16] */, void* stream);

/* ---- joint extrinsic calibration of a rig of 2 .. 8 cameras from their corner pools -------------------------------------------
 * dcx_stereo_calibrate_pool over n_cams rigidly mounted cameras with known models and one corner pool each (DcxRigCamera), all
 * with the same `batch`: frame t of every pool shows the same board at the same instant, and a camera that did not see it then
 * has an empty frame.  Camera 0 is the reference.  Result: X_c = (rvec, T), q_c = R_c q_0 + T_c, for c = 1 .. n_cams - 1, and the
 * board's pose P_t in camera 0's frame for every timestamp used.  All fp64; deepcharuco_amd/rig.py restates the steps
 * (rig_calibrate_host_full):
 * 1. per view the mask, the checks and the solve of dcx_stereo_calibrate_pool's steps 1 - 2.  A view is usable if it is
 *    DCX_PNP_OK; a timestamp is used if at least two of its views are, whichever cameras they are.  A usable view that is alone
 *    at its timestamp is reported and takes no part.
 * 2. the camera graph, on the host from one copy of the statuses: cameras share a timestamp where both are usable; camera 0 is
 *    placed, then each placed camera, in placement order, takes in ascending order every camera not placed yet that shares a
 *    timestamp with it, as its child.  Per tree edge (a -> c) dcx_stereo_calibrate_pool's rig init over the timestamps a and c
 *    share (lower medians of R_c,t R_a,t^T and t_c,t - R_t t_a,t, polar factor, Rodrigues), composed along the tree:
 *    X_c = Z o X_a (a child of camera 0 takes Z unchanged).  No used timestamp: DCX_RIG_NO_STAMPS; else a camera that is never
 *    placed: DCX_RIG_DISCONNECTED.
 * 3. P_t starts at X_c^-1 o pose_{c,t} of the timestamp's lowest-numbered usable camera c (camera 0: its own pose, unchanged).
 * 4. joint Levenberg-Marquardt over all X_c and every used P_t with dcx_stereo_calibrate_pool's rules, each step by block
 *    elimination of the timestamps' 6x6 pose blocks and one Cholesky of 6 (n_cams - 1) rows.
 * The entry point SYNCHRONISES `stream` (the statuses, the edges' R_t, T_t, a state word after every LM attempt) and cannot be
 * captured in a graph.  d_workspace: dcx_rig_calibrate_workspace_bytes(n_cams, batch, h_pools) bytes of device memory, 8-byte
 * aligned (DCX_E_WS if smaller); no device memory is allocated, and nothing but the workspace and the three output buffers is
 * written.  DCX_E_ARG: n_cams outside [2, 8], a refused camera or pool, a masked pool whose frames'
 * slot ranges overlap (found on the device; the outputs are then unspecified).
 * d_view_status int32 [B][n_cams]: DCX_PNP_* of view (t, camera).  d_pose f64 [B][8] = P_t as rvec(3), tvec(3), the timestamp's
 * rms over its usable views (px), their rows; all zero unless the timestamp was used and the status is DCX_RIG_OK.
 * d_view_info f64 [B][n_cams][2] = per view its rms at the solution (zero unless it took part and the status is DCX_RIG_OK) and
 * the rows it brings after its mask.  h_parents int32 [n_cams]: the tree, -1 for camera 0 and a camera that was not placed.
 * h_result f64 [8 + 6 (n_cams - 1)] = rms, accepted LM steps, attempts, timestamps used, points used (whatever the status),
 * DCX_RIG_* status, 0, 0, then X_1 .. X_{n_cams - 1} (rvec, T each); the rms and the X are zero unless DCX_RIG_OK.
 * No atomics, every sum in a fixed order: two calls on the same input give the same bits, and so do a NULL mask and a mask of
 * ones.                                                                                                                       */
#define DCX_RIG_OK            0
#define DCX_RIG_NO_STAMPS     1   /* no timestamp has two usable views */
#define DCX_RIG_DEGENERATE    2   /* a median matrix or a damped step is singular, or the cost is not finite */
#define DCX_RIG_NONFINITE     3
#define DCX_RIG_DISCONNECTED  4   /* a camera shares no timestamp with the cameras reached from camera 0 */
#define DCX_RIG_MAX_CAMERAS   8
typedef struct DcxRigCamera {
    const int32_t* d_counts;      /* the camera's corner pool, as for dcx_solve_pnp_pool */
    const int32_t* d_starts;
    const int32_t* d_rows;
    const float* d_xy;            /* NULL = use integer rows x,y */
    int pool;
    const uint8_t* d_mask;        /* [pool] by slot, or NULL */
    double camera9[9];            /* K row major, no skew */
    double dist[8];               /* the first n_dist are read */
    int n_dist;                   /* 0, 4, 5 or 8 */
} DcxRigCamera;
size_t dcx_rig_calibrate_workspace_bytes(int n_cams, int batch, const int* h_pools);   /* 0 for refused arguments */
int dcx_rig_calibrate_pool(int n_cams, const DcxRigCamera* h_cams, int batch, int col_count, int row_count, double square_len,
                           void* d_workspace, size_t workspace_bytes, int32_t* d_view_status /* [B][n_cams] DCX_PNP_* */,
                           double* d_pose /* [B][8] */, double* d_view_info /* [B][n_cams][2] */, int32_t* h_parents /* [n_cams] */,
                           double* h_result /* [8 + 6 (n_cams - 1)] */, void* stream);

/* dcx_rig_calibrate_pool over a rig whose cameras need not all be pinholes: h_models [n_cams] holds DCX_CAMERA_* per camera (NULL
 * = all pinhole).  A DCX_CAMERA_FISHEYE camera is the model of the dcx_fisheye_* entries: its DcxRigCamera carries k1..k4 in
 * dist[0..3] with n_dist = 4, or n_dist = 0 for zeros; its views are solved by dcx_fisheye_solve_pnp_pool's solver (a view with a
 * pixel outside the model is DCX_PNP_DEGENERATE) and its rows enter the joint solve through that model's projection.  Everything
 * else (steps, outputs, statuses, h_result, synchronisation, the bits' repeatability) is dcx_rig_calibrate_pool's, and
 * dcx_rig_calibrate_workspace_bytes serves this entry too: the workspace layout does not depend on the models.  With h_models
 * NULL or all DCX_CAMERA_PINHOLE the call IS dcx_rig_calibrate_pool: the same kernels, the same bits.  DCX_E_ARG also for a
 * model other than these two and for a fisheye camera with n_dist of 5 or 8.  deepcharuco_amd/rig.py states the steps
 * (rig_calibrate_host_full with `models`).                                                                                     */
int dcx_rig_calibrate_models_pool(int n_cams, const DcxRigCamera* h_cams, const int* h_models /* [n_cams]; NULL = all pinhole */,
                                  int batch, int col_count, int row_count, double square_len, void* d_workspace,
                                  size_t workspace_bytes, int32_t* d_view_status /* [B][n_cams] DCX_PNP_* */,
                                  double* d_pose /* [B][8] */, double* d_view_info /* [B][n_cams][2] */,
                                  int32_t* h_parents /* [n_cams] */, double* h_result /* [8 + 6 (n_cams - 1)] */, void* stream);

/* ---- the board's pose from every camera of a calibrated rig -------------------------------------------------------------------
 * What follows dcx_rig_calibrate_pool every frame afterwards: with the rig held fixed, h_rig = X_1 .. X_{n_cams - 1} as (rvec, T)
 * each (q_c = R_c q_0 + T_c; finite, DCX_E_ARG otherwise), the board's pose P_t in camera 0's frame per timestamp, from every row
 * any of the n_cams cameras saw then.  The cameras, pools, masks and h_models are dcx_rig_calibrate_models_pool's, and what that
 * entry refuses with DCX_E_ARG this one does.  Every timestamp is solved on its own.  All fp64; deepcharuco_amd/rig.py restates the
 * steps (rig_pose_host_full):
 * 1. per view the mask, the checks and the solve of dcx_rig_calibrate_pool's step 1: d_view_status, the view's own pose.
 * 2. the rows of a view CONTRIBUTE, whatever its status, if it is not DCX_PNP_TRUNCATED, keeps at least one row, every kept id is
 *    on the board and, for a fisheye camera, every kept pixel is inside the model: a DCX_PNP_TOO_FEW view of 1 to 3 rows does, a
 *    DCX_PNP_DEGENERATE view of collinear rows does.  Otherwise none of its rows do.
 * 3. every DCX_PNP_OK view is a seed, P = X_c^-1 o pose_{c,t} (camera 0: its own pose, unchanged), scored by the joint cost there:
 *    the squared pixel residual over every contributing row of every camera, +inf if a row is not in front of its camera.  The
 *    lowest score starts, the lowest camera among equals.  No seed: DCX_PNP_TOO_FEW (no view solves on its own; there is no minimal
 *    solver across cameras); every score +inf: DCX_PNP_DEGENERATE.
 * 4. dcx_solve_pnp_pool's Levenberg-Marquardt, unchanged (at most 20 accepted steps, stop at |dp| / |p| < FLT_EPSILON, the same
 *    DEGENERATE / NONFINITE endings), over the 6 parameters of P_t on the joint cost; a row of camera c >= 1 sees P_t through X_c.
 * Two launches on `stream` after the overlap / index kernels; NO synchronisation, no allocation, no atomics: the call can be
 * captured in a graph (the cameras and h_rig are copied into the kernel arguments at the call), and two calls on the same input
 * give the same bits, as do a NULL mask and a mask of ones.  d_workspace: dcx_rig_pose_workspace_bytes(n_cams, batch, h_pools)
 * bytes of device memory, 8-byte aligned (DCX_E_WS if smaller); nothing but the workspace and the six output buffers is written.
 * A masked pool whose frames' slot ranges overlap is found on the device, where the call cannot answer any more: d_head[0] = 1
 * (else 0; d_head[1] is reserved and written 0), every status and view status is DCX_PNP_TRUNCATED and everything else zero.
 * d_status int32 [B]: DCX_PNP_* per timestamp.  d_pose f64 [B][8] = P_t as rvec(3), tvec(3), rms over the contributing rows (px),
 * accepted LM steps; all zero unless the status is DCX_PNP_OK.  d_info int32 [B][2] = the camera whose pose started the solve (-1:
 * none), the contributing rows.  d_view_status int32 [B][n_cams].  d_view_info f64 [B][n_cams][2] = the view's rms at the solution
 * (zero unless it contributed and the status is DCX_PNP_OK), the rows it brings after its mask.                                 */
size_t dcx_rig_pose_workspace_bytes(int n_cams, int batch, const int* h_pools);   /* 0 for refused arguments */
int dcx_rig_pose_pool(int n_cams, const DcxRigCamera* h_cams, const int* h_models /* NULL = all pinhole */,
                      const double* h_rig /* [n_cams - 1][6]: rvec, T of X_1 .. */, int batch, int col_count, int row_count,
                      double square_len, void* d_workspace, size_t workspace_bytes, int32_t* d_head /* [2] */,
                      int32_t* d_status /* [B] */, double* d_pose /* [B][8]: rvec, tvec, rms, iterations */,
                      int32_t* d_info /* [B][2]: seed camera, rows */, int32_t* d_view_status /* [B][C] */,
                      double* d_view_info /* [B][C][2]: rms, kept rows */, void* stream);

/* ---- stereo rectification: the undistort + rectify map, the remap of u8 frames, the corner pool in rectified coordinates ------
 * What follows dcx_stereo_calibrate_pool: with the rig's rectifying transforms (R1, R2, P1, P2 of
 * deepcharuco_amd/rectify.py:stereo_rectify_host, Bouguet's construction as cv2.stereoRectify with CALIB_ZERO_DISPARITY; host
 * code, once per rig) the three calls put both cameras' frames and corners on common epipolar rows.  Cameras as for
 * dcx_solve_pnp_pool (h_camera9 without skew, n_dist = 0, 4, 5 or 8; DCX_E_ARG otherwise).  h_R9: a 3x3 rotation, row major, NULL =
 * identity.  h_P12: a 3x4 projection, row major, of which the left 3x3 is used (P[0][1] must be 0, P[0][0] and P[1][1] not),
 * NULL = K; with both NULL the calls undistort a single camera.  All host arguments are copied into the kernel arguments at the
 * call.  Each call is one launch on `stream`: no allocation, no synchronisation, no atomics, so two calls give the same bits and
 * every call can be captured in a hipGraph.  deepcharuco_amd/rectify.py restates the steps.
 *
 * dcx_undistort_rectify_map (cv2.initUndistortRectifyMap; fp64, once per camera and rig): d_map int32 [height][width][2],
 * 8-byte aligned here and in dcx_remap_u8 (DCX_E_ARG otherwise).  For
 * output pixel (u, v): x = (u - P02) / P00, y = (v - P12) / P11, q = R^T (x, y, 1); the entry is rint(32 m) (5 fractional bits,
 * ties to even) with m the camera's projection of (q_x / q_z, q_y / q_z) through its distortion model, or INT32_MIN in both
 * components ("outside") if q_z <= 0 or m is not finite or beyond +-32768 px.  The output size need not be the source's.
 *
 * dcx_rectify_points_pool (cv2.undistortPoints with R and P; fp64): every SLOT i < pool of a corner pool, one lane each, whatever
 * frame it belongs to: the pixel d_xy[i] (or, with d_xy == NULL, the integer x, y of d_rows[i]) -> d_out f64 [pool][2] =
 * P R undistort(pixel).  Undistortion is Newton on the distortion model's analytic 2x2 Jacobian from the normalised pixel, until
 * both components of a step are below 1e-15, at most 20 steps (NOT the 5 fixed-point rounds of dcx_solve_pnp_pool: those are
 * up to 4.8e-3 px off over a 320x240 frame with k1 = -0.25); NaN if it has not converged or the rotated z <= 0.  pool = 0 is
 * allowed (nothing is launched).
 *
 * dcx_remap_u8 (cv2.remap INTER_LINEAR, BORDER_CONSTANT; the per-frame hot path): batch frames d_src (u8, `channels` = 1 or 3
 * interleaved, rows `pitch` bytes apart, frames `frame_stride` bytes apart, both in bytes as for dcx_bgr2gray) through ONE map ->
 * d_out u8 [batch][out_h][out_w][channels], dense.  Integer arithmetic, bit-exact against rectify.py:remap_host: with (mx, my) the
 * entry, x0 = mx >> 5, y0 = my >> 5 (arithmetic), fx = mx & 31, fy = my & 31, taps p00 = (x0, y0), p10 = (x0+1, y0),
 * p01 = (x0, y0+1), p11 = (x0+1, y0+1), each tap outside the source reading `border` (0..255; so does an "outside" entry),
 * out = ((32-fx)(32-fy) p00 + fx (32-fy) p10 + (32-fx) fy p01 + fx fy p11 + 512) >> 10 per channel.  This is cv2's 5-bit scheme
 * with the weights as exact products; cv2 rounds its weight table and patches it to sum to 2^15, so its bits are not claimed.
 * pitch * src_h must fit an int32 (DCX_E_SHAPE).                                                                              */
int dcx_undistort_rectify_map(const double* h_camera9, const double* h_dist, int n_dist,
                              const double* h_R9 /* NULL = identity */, const double* h_P12 /* NULL = K */,
                              int width, int height, int32_t* d_map /* [height][width][2] */, void* stream);
int dcx_rectify_points_pool(const int32_t* d_rows, const float* d_xy /* NULL = use integer rows x,y */, int pool,
                            const double* h_camera9, const double* h_dist, int n_dist,
                            const double* h_R9 /* NULL = identity */, const double* h_P12 /* NULL = K */,
                            double* d_out /* [pool][2] */, void* stream);
int dcx_remap_u8(const uint8_t* d_src, long frame_stride, int pitch, int src_h, int src_w, int channels /* 1 or 3 */,
                 const int32_t* d_map, int out_h, int out_w, int batch, int border, uint8_t* d_out, void* stream);

/* ---- the fisheye camera model (cv2.fisheye's documented model, skew 0): pose, calibration, undistortion ----------------------
 * For a camera-frame point (X, Y, Z): a = X/Z, b = Y/Z, r = sqrt(a^2 + b^2), theta = atan r,
 * theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), x' = (theta_d / r) a, y' = (theta_d / r) b,
 * u = fx x' + cx, v = fy y' + cy.  As everywhere here a point must have Z > 0: the field of view is under 180 degrees.  theta_d / r
 * and its derivative come from their series below r = 1e-4, so a point on the optical axis is a valid input.  The inverse is
 * Newton on theta (1 + k1 theta^2 + ...) - theta_d from theta = theta_d until a step is below 1e-15, at most 20 steps; a pixel is
 * OUTSIDE if Newton does not converge or theta is not in [0, pi/2).  h_camera9 as for dcx_solve_pnp_pool (no skew, finite, non-zero
 * focal lengths; DCX_E_ARG otherwise); h_dist4 = k1, k2, k3, k4 (finite), NULL = zeros.  All fp64; deepcharuco_amd/fisheye.py
 * restates every step and csrc/dcx_fisheye_dev.h holds the model.
 *
 * dcx_fisheye_solve_pnp_pool: dcx_solve_pnp_pool with this camera: one wavefront per frame, the same pool, checks, DCX_PNP_* codes
 * and [B][8] pose words; a frame with a pixel outside the model is DCX_PNP_DEGENERATE.  One launch on `stream`: no allocation, no
 * synchronisation, capturable in a hipGraph.
 *
 * dcx_fisheye_calibrate_pool (cv2.fisheye.calibrate's role, planar target): pool, per-view checks, d_view_status, d_pose and the
 * DCX_CALIB_* codes as for dcx_calibrate_pool.  Start: principal point ((w-1)/2, (h-1)/2); fx = fy = focal0, or max(w, h) / 2 if
 * focal0 is not > 0 (+inf: DCX_E_ARG); k = 0; every view's pose by dcx_fisheye_solve_pnp_pool's solve at that camera (a view it
 * refuses is left out and reported).  Then joint Levenberg-Marquardt over fx, fy, cx, cy, k1..k4 and every used view's pose with
 * dcx_calibrate_pool's rules and block elimination, at most 100 accepted steps, stop at |dp|/|p| < DBL_EPSILON.
 * h_result f64 [16] = fx, fy, cx, cy, k1, k2, k3, k4, 0, rms, accepted LM steps, attempts, views used, points used, DCX_CALIB_*
 * status, 0; the first ten are zero unless DCX_CALIB_OK.  d_workspace: dcx_fisheye_calibrate_workspace_bytes(batch) bytes of
 * device memory (DCX_E_WS if smaller); nothing is allocated.  Like dcx_calibrate_pool this entry point SYNCHRONISES `stream` (the
 * LM loop runs on the host and reads a state word after every attempt) and cannot be captured in a graph.  No atomics: two calls
 * on the same input give the same bits.
 *
 * dcx_fisheye_undistort_rectify_map / dcx_fisheye_rectify_points_pool: dcx_undistort_rectify_map / dcx_rectify_points_pool with
 * the ray through this model (cv2.fisheye.initUndistortRectifyMap / undistortPoints): the same R and P, the same int32 map in
 * 1/32 px with INT32_MIN for outside (q_z <= 0, a source position that is not finite or beyond +-32768 px), which dcx_remap_u8
 * reads unchanged; the same f64 [pool][2] output, NaN for a pixel outside the model or a rotated z <= 0.                      */
int dcx_fisheye_solve_pnp_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows,
                               const float* d_xy /* NULL = use integer rows x,y */, int batch, int pool,
                               int col_count, int row_count, double square_len,
                               const double* h_camera9, const double* h_dist4 /* NULL = zeros */,
                               int32_t* d_status, double* d_pose /* [B][8] */, void* stream);

/* dcx_solve_pnp_ransac_pool on a fisheye camera (h_camera9, h_dist4 as for dcx_fisheye_solve_pnp_pool): the same sampler, score
 * order, mask format, info words, statuses, workspace (dcx_solve_pnp_ransac_workspace_bytes serves this entry too) and capture
 * rules.  The sample's four pixels go through the model's undistort; a sample with a pixel outside the model has no hypothesis
 * (score -1); rows are scored by forward projection through the model; the winner's inliers go to the unchanged solver, which
 * answers DCX_PNP_DEGENERATE if one of them lies outside the model.  No allocation, no sync, capturable.  A workspace smaller
 * than dcx_solve_pnp_ransac_workspace_bytes is DCX_E_WS here (dcx_solve_pnp_ransac_pool answers DCX_E_ARG).                   */
int dcx_fisheye_solve_pnp_ransac_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy,
                                      int batch, int pool, int col_count, int row_count, double square_len,
                                      const double* h_camera9, const double* h_dist4, int iterations, double reproj_error,
                                      int min_inliers, unsigned seed, void* d_workspace, size_t workspace_bytes, int32_t* d_status,
                                      double* d_pose, int32_t* d_info, uint8_t* d_inliers, void* stream);
size_t dcx_fisheye_calibrate_workspace_bytes(int batch);
int dcx_fisheye_calibrate_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows,
                               const float* d_xy /* NULL = use integer rows x,y */, int batch, int pool,
                               int col_count, int row_count, double square_len, int image_width, int image_height,
                               double focal0 /* not > 0: max(w, h) / 2 */, void* d_workspace, size_t workspace_bytes,
                               int32_t* d_view_status /* [B] DCX_PNP_* */, double* d_pose /* [B][8] */,
                               double* h_result /* [16] */, void* stream);
int dcx_fisheye_undistort_rectify_map(const double* h_camera9, const double* h_dist4,
                                      const double* h_R9 /* NULL = identity */, const double* h_P12 /* NULL = K */,
                                      int width, int height, int32_t* d_map /* [height][width][2] */, void* stream);
int dcx_fisheye_rectify_points_pool(const int32_t* d_rows, const float* d_xy /* NULL = use integer rows x,y */, int pool,
                                    const double* h_camera9, const double* h_dist4,
                                    const double* h_R9 /* NULL = identity */, const double* h_P12 /* NULL = K */,
                                    double* d_out /* [pool][2] */, void* stream);

/* ---- how well a calibration is determined: the covariances of the intrinsics and of the views' poses -------------------------
 * cv2.calibrateCameraExtended's stdDeviationsIntrinsics / stdDeviationsExtrinsics, for a model solved by dcx_calibrate_pool,
 * dcx_calibrate_ransac_pool (model DCX_CAMERA_PINHOLE, h_theta [9] = fx fy cx cy k1 k2 p1 p2 k3) or dcx_fisheye_calibrate_pool
 * (DCX_CAMERA_FISHEYE, h_theta [8] = fx fy cx cy k1 k2 k3 k4); another model code is DCX_E_ARG.  Pool arguments, object and image
 * points as for dcx_calibrate_pool.  d_view_status [B]: a view takes part where it is DCX_PNP_OK; d_pose [B][8] as the calibrations
 * write it (words 0..5 = rvec, tvec are read); d_mask [pool] by slot, the format of dcx_calibrate_ransac_pool's d_inliers, drops the
 * rows whose byte is 0 (NULL: every row).  None of the inputs is written.  h_theta is read at the call and passed to the kernels
 * by value.  All fp64; deepcharuco_amd/calib.py restates the definition (calibration_uncertainty_host).  With the undamped normal
 * blocks of the calibration at (theta, poses), U_i 6x6, W_i NG x 6 per used view and V NG x NG over their kept rows:
 *   S = V - sum W_i U_i^-1 W_i^T, Y_i = U_i^-1 W_i^T, dof = 2 points - NG - 6 views, sigma^2 = sum |r|^2 / dof (the textbook
 *   estimator: residuals minus parameters; rescale by dof / another divisor for another convention),
 *   cov_intrinsics = sigma^2 S^-1, cov_pose_i = sigma^2 (U_i^-1 + Y_i S^-1 Y_i^T), standard deviations = the diagonals' roots.
 * d_global f64 [DCX_COV_GLOBAL_WORDS], every word written: cov_intrinsics NG x NG row major (row stride NG) from DCX_COV_COV, the NG
 * standard deviations from DCX_COV_STD, then sigma^2, dof, points (kept rows of the used views), views used, the DCX_COV_* status
 * and 0.  d_pose_cov f64 [B][DCX_COV_POSE_WORDS]: cov_pose_i 6x6 row major in the order rvec, tvec (cv2's), then its 6 standard
 * deviations; zeros for a view that was not used.  Everything but the status, dof, points and views is zero unless DCX_COV_OK.
 * A used view whose slots leave the pool counts as DCX_COV_SINGULAR (its slots are not read).
 * d_workspace: dcx_calibrate_uncertainty_workspace_bytes(batch) bytes of device memory (DCX_E_WS if smaller; one size for both
 * models); nothing is allocated and nothing but the workspace and the two outputs is written.  Four launches on `stream`, every
 * sum in a fixed order, no atomics: two calls give the same bits.  UNLIKE the calibrations there is no host loop and NO
 * synchronisation: the call can be captured in a graph.                                                                      */
#define DCX_COV_OK        0
#define DCX_COV_NO_VIEWS  1   /* no view is DCX_PNP_OK */
#define DCX_COV_NO_DOF    2   /* dof <= 0: no more residuals than parameters */
#define DCX_COV_SINGULAR  3   /* a U_i or S is not positive definite, a point is not in front of the camera, or a value is not finite */
#define DCX_COV_COV       0   /* offsets into d_global */
#define DCX_COV_STD       81
#define DCX_COV_SIGMA2    90
#define DCX_COV_DOF       91
#define DCX_COV_POINTS    92
#define DCX_COV_VIEWS     93
#define DCX_COV_STATUS    94
#define DCX_COV_GLOBAL_WORDS 96
#define DCX_COV_POSE_WORDS   42
size_t dcx_calibrate_uncertainty_workspace_bytes(int batch);
int dcx_calibrate_uncertainty_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows,
                                   const float* d_xy /* NULL = use integer rows x,y */, int batch, int pool,
                                   int col_count, int row_count, double square_len, int model /* DCX_CAMERA_* */,
                                   const double* h_theta /* [9] or [8] */, const int32_t* d_view_status /* [B] */,
                                   const double* d_pose /* [B][8] */, const uint8_t* d_mask /* [pool] or NULL */,
                                   void* d_workspace, size_t workspace_bytes, double* d_global /* [DCX_COV_GLOBAL_WORDS] */,
                                   double* d_pose_cov /* [B][DCX_COV_POSE_WORDS] */, void* stream);

/* ---- how well a rig is determined: the covariances of the rig's extrinsics and of the board poses ------------------------------
 * What dcx_calibrate_uncertainty_pool is to dcx_calibrate_pool, for a rig solved by dcx_stereo_calibrate_pool (n_cams = 2) or
 * dcx_rig_calibrate_pool / _models_pool: the covariance of X_1 .. X_{n_cams - 1} (rvec, T each) and of every used timestamp's P_t,
 * GIVEN THE CAMERA MODELS: the intrinsics and distortion coefficients are held fixed, as those calibrations hold them.  The
 * cameras, pools, masks (DcxRigCamera.d_mask) and h_models are dcx_rig_calibrate_models_pool's, and what that entry refuses with
 * DCX_E_ARG this one does; h_rig [n_cams - 1][6] is dcx_rig_pose_pool's (read at the call, passed to the kernels by value).
 * d_view_status int32 [B][n_cams] and d_pose f64 [B][8] as the calibration wrote them (words 0..5 of a used timestamp are read): a
 * view is usable where it is DCX_PNP_OK, a timestamp is used if two of its views are.  None of the inputs is written; connectivity
 * is not checked.  All fp64; deepcharuco_amd/rig.py restates the definition (rig_uncertainty_host).  With the undamped normal blocks
 * of the rig calibration at (X, P), U_t 6x6, W_t n x 6 per used timestamp and V n x n (block diagonal), n = 6 (n_cams - 1), over
 * the kept rows of the usable views:
 *   S = V - sum W_t U_t^-1 W_t^T, Y_t = U_t^-1 W_t^T, dof = 2 points - n - 6 stamps, sigma^2 = sum |r|^2 / dof (the convention of
 *   dcx_calibrate_uncertainty_pool), cov_rig = sigma^2 S^-1, cov_pose_t = sigma^2 (U_t^-1 + Y_t S^-1 Y_t^T), standard deviations
 *   = the diagonals' roots.  The X - P cross-covariances are not reported.
 * d_global f64 [DCX_RIGCOV_GLOBAL_WORDS], ONE layout for every n_cams, every word written: cov_rig row major with row stride
 * DCX_RIGCOV_STRIDE (42) from DCX_RIGCOV_COV, in the order rvec_c, T_c per camera, cameras ascending; DCX_RIGCOV_STRIDE standard
 * deviations from DCX_RIGCOV_STD; then sigma^2, dof, points (kept rows of the usable views of the used timestamps), timestamps
 * used, the DCX_COV_* status and 0.  Entries past n are zero.  d_pose_cov f64 [B][DCX_COV_POSE_WORDS]: cov_pose_t 6x6 row major
 * (rvec, tvec), then its 6 standard deviations; zeros for a timestamp that was not used.  Everything but the status, dof, points
 * and stamps is zero unless DCX_COV_OK.  Statuses in this order: DCX_COV_NO_VIEWS (no used timestamp), DCX_COV_NO_DOF,
 * DCX_COV_SINGULAR (a U_t or S that is not positive definite, which includes a camera c >= 1 without a usable view in any used
 * timestamp; a point not in front of its camera; a kept id outside the board; a value that is not finite; a used view whose slots
 * leave its pool, which are then not read).
 * d_workspace: dcx_rig_uncertainty_workspace_bytes(n_cams, batch, h_pools) bytes of device memory, 8-byte aligned (DCX_E_WS if
 * smaller); nothing is allocated and nothing but the workspace and the two outputs is written.  Five launches on `stream`, every
 * sum in a fixed order, no atomics: two calls give the same bits, and a masked pool gives the bits of the pool with the dropped
 * rows removed (a dropped row is added as a row of zeros, so frames of a masked pool may share slots here).  No host loop and NO
 * synchronisation: the call can be captured in a graph.                                                                       */
#define DCX_RIGCOV_STRIDE  42     /* 6 (DCX_RIG_MAX_CAMERAS - 1) */
#define DCX_RIGCOV_COV     0      /* offsets into d_global */
#define DCX_RIGCOV_STD     1764
#define DCX_RIGCOV_SIGMA2  1806
#define DCX_RIGCOV_DOF     1807
#define DCX_RIGCOV_POINTS  1808
#define DCX_RIGCOV_STAMPS  1809
#define DCX_RIGCOV_STATUS  1810
#define DCX_RIGCOV_GLOBAL_WORDS 1812
size_t dcx_rig_uncertainty_workspace_bytes(int n_cams, int batch, const int* h_pools);   /* 0 for refused arguments */
int dcx_rig_uncertainty_pool(int n_cams, const DcxRigCamera* h_cams, const int* h_models /* NULL = all pinhole */,
                             const double* h_rig /* [n_cams - 1][6]: rvec, T of X_1 .. */, int batch, int col_count, int row_count,
                             double square_len, const int32_t* d_view_status /* [B][n_cams] */, const double* d_pose /* [B][8] */,
                             void* d_workspace, size_t workspace_bytes, double* d_global /* [DCX_RIGCOV_GLOBAL_WORDS] */,
                             double* d_pose_cov /* [B][DCX_COV_POSE_WORDS] */, void* stream);

/* ---- image resizing (cv2.resize): what stands in front of the detector ---------------------------------------------------------
 * dcx_resize_u8: batch frames d_src (u8, `channels` = 1 or 3 interleaved, rows `pitch` bytes apart, frames `frame_stride` bytes
 * apart, any base address: a cropped view costs nothing) -> d_out u8 [batch][out_h][out_w][channels], dense.  Channels are
 * independent.  Bit-exact against deepcharuco_amd/resize.py:resize_host, which states every step; the formulas are cv2's as
 * published and are NOT pinned against cv2.  With sw, sh the source and dw, dh the output size, per axis
 * scale = 1.0 / (dn / sn) in double (computed by this entry on the host, a kernel argument):
 *
 * interpolation 0, "nearest": sx = min(floor(dx * scale), sw - 1), the same in y, fp64.
 * interpolation 2, "area": only sw = fx dw and sh = fy dh with integers 1 <= fx, fy <= 64 (DCX_E_SHAPE otherwise); sum = the
 *   integer sum of the fx fy source pixels; fx = fy = 2: out = (sum + 2) >> 2; else out = rint(float(sum) * float(1.0 / (fx fy))),
 *   one float32 product, ties to even.
 * interpolation 1, "linear": sw = 2 dw and sh = 2 dh gives "area" (cv2's rule).  Otherwise per axis f = float((d + 0.5) * scale
 *   - 0.5) (product and difference each rounded to double, no fused multiply-add), s = floor(f), f = f - float(s) in float32.
 *   In x: s < 0 gives f = 0, s = 0; s >= sw - 1 gives f = 0, s = sw - 1; the taps are s and min(s + 1, sw - 1).  In y the rows are
 *   clip(s, 0, sh - 1) and clip(s + 1, 0, sh - 1) and f stays.  Coefficients c0 = rint(float(1 - f) * 2048), c1 = rint(f * 2048)
 *   in float32, ties to even, each on its own (a0, a1 in x; b0, b1 in y).  r = S[x0] a0 + S[x1] a1 on both rows (int32), then
 *   out = (((b0 (r0 >> 4)) >> 16) + ((b1 (r1 >> 4)) >> 16) + 2) >> 2.  A reduction reads the two tap rows only.
 *
 * DCX_E_ARG: a null pointer, channels not 1 or 3, an interpolation not 0, 1 or 2, a negative frame_stride.  DCX_E_SHAPE: src_h,
 * src_w, out_h, out_w or batch outside 1 .. 32768, pitch < src_w * channels, pitch * src_h beyond an int32, a refused area
 * factor.  Every refusal comes before anything is launched.  One launch on `stream`: no workspace, no allocation, no
 * synchronisation, no atomics, so two calls give the same bits and a call can be captured in a hipGraph.                      */
int dcx_resize_u8(const uint8_t* d_src, long frame_stride, int pitch, int src_h, int src_w, int channels /* 1 or 3 */,
                  int out_h, int out_w, int batch, int interpolation /* 0 nearest, 1 linear, 2 area */, uint8_t* d_out,
                  void* stream);

/* dcx_resize_area_u8: cv2's general INTER_AREA for shrinking ("area_any": a box filter with fractional end taps), frames and
 * output laid out as for dcx_resize_u8.  Bit-exact against deepcharuco_amd/resize.py:resize_host(..., "area_any"); cv2's formula
 * as published (imgproc resize.cpp: computeResizeAreaTab and the general area invoker), NOT pinned against cv2.
 *
 * 1. Routing (cv2's fast-path rule): sw = fx dw AND sh = fy dh with integer factors gives dcx_resize_u8's "area", bit for bit,
 *    through the same kernels (identity and 2 x 2 included).  Otherwise BOTH axes take the general path, also one whose own factor
 *    is an integer.
 * 2. The tap table of an axis, all in double, each operation rounded once, no fused multiply-add, scale = 1.0 / (dn / sn).  For
 *    output index d: f1 = d * scale, f2 = f1 + scale, cell = min(scale, sn - f1); s1 = ceil(f1), s2 = min(floor(f2), sn - 1),
 *    s1 = min(s1, s2).  Taps in this order: if s1 - f1 > 1e-3: (s1 - 1, float((s1 - f1) / cell)); for s in s1 .. s2 - 1:
 *    (s, float(1.0 / cell)); if f2 - s2 > 1e-3: (s2, float(min(min(f2 - s2, 1.0), cell) / cell)).
 * 3. A pixel, channels independent, float32 throughout, every product and every sum rounded on its own.  For each y-tap (sy, b)
 *    in order: h = the sum over the x-taps (sx, a) in order of float(S[sy][sx]) * a, starting from the first product; v = b * h
 *    for the first y-tap, v = v + b * h for the others; out = clip(rint(v), 0, 255), ties to even.  Horizontal first, then
 *    vertical: cv2's order, and part of the definition.
 *
 * DCX_E_ARG: a null pointer, channels not 1 or 3, a negative frame_stride.  DCX_E_SHAPE: src_h, src_w, out_h, out_w or batch
 * outside 1 .. 32768, pitch < src_w * channels, pitch * src_h beyond an int32, out_h > src_h or out_w > src_w (area does not
 * enlarge), src_h > 64 out_h or src_w > 64 out_w.  Every refusal comes before anything is launched.  One launch on `stream`: no
 * workspace, no allocation, no synchronisation, no atomics, so two calls give the same bits and a call can be captured in a
 * hipGraph.                                                                                                                    */
int dcx_resize_area_u8(const uint8_t* d_src, long frame_stride, int pitch, int src_h, int src_w, int channels /* 1 or 3 */,
                       int out_h, int out_w, int batch, uint8_t* d_out, void* stream);

/* ---- dense stereo matching on a rectified pair, and the disparity map as 3-D points ------------------------------------------
 * What follows dcx_remap_u8: semi-global matching (what cv2.StereoSGBM is called for) over 9 x 7 census costs, integer throughout
 * and bit-exact against deepcharuco_amd/disparity.py:sgm_host, which states every step.  d_left is rectified camera 0 and d_right
 * rectified camera 1 of a horizontal rig (a vertical rig passes transposed frames); the disparity d = x_left - x_right is the d of
 * Q.  Both are u8 gray frames, rows pitch_* bytes apart and frames frame_stride_* bytes apart, each image its own (pitch >= width,
 * else DCX_E_SHAPE).  num_disparities D is 64, 128 or 256, 1 <= width <= 4096, 1 <= height <= 32768 (DCX_E_SHAPE);
 * 0 <= p1 <= p2 <= 255, 0 <= uniqueness < 100, -2047 <= min_disparity and min_disparity + D <= 2047 (DCX_E_ARG);
 * lr_max_diff < 0 switches the left-right check off.  d_disp16 int16 [batch][height][width], dense: the disparity times 16,
 * 16 (min_disparity - 1) where invalid (cv2's convention).
 *
 * Steps: census words (62 bits: neighbour < centre, rows top to bottom, columns left to right, the first neighbour most
 * significant, edge-replicated); C(y, x, d) = popcount(cenL[y][x] ^ cenR[y][clamp(x - m - d, 0, W - 1)]); four paths (both
 * directions along rows and columns) L(p, d) = C + min(L(q, d), L(q, d - 1) + p1, L(q, d + 1) + p1, M + p2) - M with
 * M = min_k L(q, k), summed into S (u16); the winner d* = the lowest d of the smallest S; invalid if x - m - d* leaves the row, if
 * some d with |d - d*| > 1 has S[d] (100 - uniqueness) < S[d*] 100, or if the right view's winner at x - m - d* (the lowest d of
 * the smallest S(y, xr + m + d, d)) is more than lr_max_diff from d*; sub-pixel off = floor((16 num + den) / (2 den)) with
 * num = S[d*-1] - S[d*+1], den = S[d*-1] + S[d*+1] - 2 S[d*], where 0 < d* < D - 1 and den > 0; the value is 16 (m + d*) + off.
 *
 * d_workspace (8-byte aligned, DCX_E_ARG otherwise): dcx_sgm_workspace_bytes(batch, ...) = batch * height * width * (16 + 2 D)
 * bytes take the batch in one pass of four launches; with fewer bytes the batch is taken in chunks of as many frames as fit, and
 * with less than one frame's the call is refused (DCX_E_WS).  Launches on `stream` only: no allocation, no synchronisation, no
 * global atomics, so two calls give the same bits and a call can be captured in a hipGraph.
 *
 * dcx_sgm_u8_paths is dcx_sgm_u8 with the number of aggregation paths, 4 or 8 (anything else DCX_E_ARG, before anything is
 * launched).  With 4 it is dcx_sgm_u8: the same launches, the same bits.  With 8 S also receives the four diagonal paths,
 * (dy, dx) = (+1, +1), (-1, -1), (+1, -1), (-1, +1): the same recursion with q = p - (dy, dx), a path beginning (L = C) at every
 * pixel whose q lies outside the frame; S <= 8 (62 + 255) still fits its u16.  Two more launches per chunk, one per diagonal
 * family, in the same workspace.
 *
 * dcx_disparity_to_points (cv2.reprojectImageTo3D): one thread per pixel; with d = disp16 / 16 and h = Q (x, y, d, 1)^T, each row
 * summed left to right in fp64 without contraction, d_xyz f32 [batch][height][width][3] = h[0..2] / h[3], rounded to float once;
 * NaN where disp16 < 16 min_disparity (invalid) or disp16 == 0.  h_Q16: 4x4 row major, finite (DCX_E_ARG otherwise), copied into
 * the kernel arguments at the call.                                                                                           */
size_t dcx_sgm_workspace_bytes(int batch, int height, int width, int num_disparities);   /* 0 for refused arguments */
int dcx_sgm_u8(const uint8_t* d_left, long frame_stride_l, int pitch_l, const uint8_t* d_right, long frame_stride_r, int pitch_r,
               int batch, int height, int width, int min_disparity, int num_disparities, int p1, int p2, int uniqueness,
               int lr_max_diff, int16_t* d_disp16, void* d_workspace, size_t workspace_bytes, void* stream);
int dcx_sgm_u8_paths(const uint8_t* d_left, long frame_stride_l, int pitch_l, const uint8_t* d_right, long frame_stride_r, int pitch_r,
                     int batch, int height, int width, int min_disparity, int num_disparities, int p1, int p2, int uniqueness,
                     int lr_max_diff, int paths /* 4 or 8 */, int16_t* d_disp16, void* d_workspace, size_t workspace_bytes,
                     void* stream);
int dcx_disparity_to_points(const int16_t* d_disp16, int batch, int height, int width, int min_disparity,
                            const double* h_Q16 /* 4x4 row major */, float* d_xyz /* [batch][height][width][3] */, void* stream);

/* ---- the speckle filter for disparity maps (cv2.filterSpeckles) -----------------------------------------------------------------
 * What follows dcx_sgm_u8 (cv2's StereoSGBM calls it with new_val = 16 (min_disparity - 1), max_speckle_size = speckleWindowSize,
 * max_diff = 16 speckleRange).  d_in int16 [batch][height][width], dense, each frame on its own.  Pixels equal to new_val are never
 * touched and belong to no component; among the others two 4-neighbours are joined when their values differ by at most max_diff;
 * every pixel of a connected component of at most max_speckle_size pixels becomes new_val in d_out (max_speckle_size = 0 copies).
 * All integer and bit-exact against deepcharuco_amd/disparity.py:filter_speckles_host: the result depends on the components'
 * sizes only, so on no order of execution, and two calls give the same bits.  d_out may equal d_in; any other overlap is the
 * caller's error.  new_val an int16 value, max_speckle_size >= 0, 0 <= max_diff <= 65535 (DCX_E_ARG); batch >= 1,
 * 1 <= height, width <= 2^20 and height * width <= 2^30 (DCX_E_SHAPE); d_in, d_out 2-byte and d_workspace 8-byte aligned (DCX_E_ARG).
 *
 * d_workspace: dcx_filter_speckles_workspace_bytes(batch, ...) = batch * height * width * 8 bytes (a 32-bit label and a 32-bit
 * size per pixel) take the batch in one pass; with fewer bytes the batch is taken in chunks of as many frames as fit, and with
 * less than one frame's the call is refused (DCX_E_WS).  One frame of dcx_sgm_u8's workspace holds at least 18 frames of this one,
 * so the matcher's workspace serves the filter that follows it.  Four launches per chunk on `stream` (labels of 32 x 32 tiles in
 * LDS; unions across tile edges by global atomics; roots and sizes; the rewrite): no allocation, no synchronisation, no kernel
 * waits for another workgroup, and a call can be captured in a hipGraph.                                                       */
size_t dcx_filter_speckles_workspace_bytes(int batch, int height, int width);   /* batch * H * W * 8; 0 for refused shapes */
int dcx_filter_speckles_s16(const int16_t* d_in, int16_t* d_out, int batch, int height, int width, int new_val,
                            int max_speckle_size, int max_diff, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- stage-level entry point for kernel tests / roofline measurement -------------------
 * One 3x3 (or 1x1) convolution + bias [+ eval-BN + ReLU] [+ 2x2 max-pool] on C4 tensors
 * using the same MFMA kernel the networks use.  h_* are host arrays in PyTorch layout;
 * the call packs/uploads them (synchronously) and then enqueues the kernel on `stream`.
 * ups: input is read through a nearest x2 up-sampling.  d_in C4 [N][cin/4][Hin][Win][4],
 * d_out C4 [N][ceil(cout/4)][Hout][Wout][4].                                              */
int dcx_conv_layer(const float* d_in, int n, int cin, int hin, int win,
                   const float* h_weight_oihw, const float* h_bias,
                   const float* h_bn_gamma, const float* h_bn_beta,
                   const float* h_bn_mean, const float* h_bn_var,
                   int cout, int ksize, int pad, int ups, int pool, int relu,
                   float* d_out, void* stream);
/* NCHW <-> C4 layout converters (tests, API edges). c need not be a multiple of 4 (zero fill). */
int dcx_nchw_to_c4(const float* d_nchw, int n, int c, int h, int w, float* d_c4, void* stream);
int dcx_c4_to_nchw(const float* d_c4, int n, int c, int h, int w, float* d_nchw, void* stream);

/* ---- instrumentation: per-stage device time of the last dcx_infer_batch() ---------------
 * When enabled, the pipeline records hipEvents on its stream around each stage; after the
 * stream has been synchronised by the caller, dcx_last_timings() returns milliseconds:
 * [0] detector conv stack, [1] fused tail (1x1 heads + arg-max + ordered compaction into the corner pool), [2] RefineNet INCLUDING
 * the patch gather (its conv1a reads the 24x24 windows out of the frames since round 3), [3] total.  */
int dcx_set_timing(int enabled);
int dcx_get_timing(void);            /* 1 while per-stage timing is on (callers that capture hipGraphs must launch eagerly then) */
int dcx_last_timings(float* h_ms4);

/* name of the kernel instantiation the tile cost model selects for a launch shape (host only, no GPU needed);
 * epi: 0 = BN+ReLU, 1 = raw (1x1 heads), 2 = RefineNet head; "" when no instantiation fits */
const char* dcx_conv_pick_name(int n, int cin, int ho, int wo, int cout, int ks, int pool, int epi);
/* same for a layer whose input is read through a nearest x2 up-sampling (ho x wo = output size = 2 x the stored input) */
const char* dcx_conv_pick_name_ups(int n, int cin, int ho, int wo, int cout, int ks, int pool, int epi, int ups);

/* ---- kernel families / deterministic mode -------------------------------------------------
 * The kernel family of a layer (= the fp32 summation order of its outputs: direct implicit GEMM, 2-D Winograd F(2x2,3x3),
 * or phases x Winograd F(2x2,2x2) behind an up-sampling) depends on the LAYER only, never on the batch size or launch size:
 * a frame's results are bit-identical alone and inside any batch.  dcx_set_deterministic(1) (or
 * DCX_DETERMINISTIC=1 in the environment) forces the direct family everywhere -- every multiply-add of the layers as written,
 * the A/B reference of the Winograd families -- at about 0.5x the default throughput.  Process-global; callers that hold
 * captured hipGraphs must re-capture after switching (the Python layer does).                                          */
int dcx_set_deterministic(int enabled);
int dcx_get_deterministic(void);

/* ---- hand-off mode of the detector tail's fused compaction (csrc/dcx_tail.hip) --------------
 * 0 (default): the frame's last work item learns about the other work items' codes without fences -- write-through (sc1) stores
 * drained by s_waitcnt vmcnt(0), one relaxed agent-scope ticket, agent-scope (sc1) loads: gfx942 / gfx950 behaviour, soaked by
 * tests/test_gpu_parity.py::test_tail_handoff_is_never_stale.  1 (or DCX_TAIL_FENCE=1 in the environment): the release / acquire
 * pair the HIP memory model defines (__threadfence() on both sides, ~4x the kernel's time): the A/B for new ROCm drops.
 * Same results either way.  Process-global; captured hipGraphs keep the mode they were captured with.                  */
int dcx_set_tail_fence(int enabled);
int dcx_get_tail_fence(void);

/* ---- per-XCD item shares (speed only; the work items and their bits do not change) ---------
 * The convolution kernels are persistent grids whose workgroups walk one contiguous share of the item list per XCD (8 XCDs, each
 * with its own L2).  The XCDs of one chip do not run this load equally fast (3-6 % apart), and a launch ends with its slowest XCD:
 * dcx_calibrate_xcd measures them (`rounds` ~0.8 ms launches of the dominant kernel on a synthetic conv1b-sized layer; synchronous,
 * set-up code: GPU warm, outside timed regions and hipGraph capture) and sets the shares accordingly; dcx_set_xcd_weights sets
 * them by hand (8 relative speeds, NULL = equal; more than 25 % from equal is refused with DCX_E_ARG); dcx_get_xcd_weights returns
 * them (1.0 = an equal share).  Per device (the current one), process-global; hipGraphs keep the shares they were captured with:
 * the shares live in a ring of 256 device tables per device, so a graph captured through this API must be re-captured before
 * its device's shares are set 256 more times.                                                                                      */
int dcx_calibrate_xcd(int rounds, float* w8_out, void* stream);
int dcx_set_xcd_weights(const float* w8);
int dcx_get_xcd_weights(float* w8);

/* ---- instrumentation: per-launch profile of the MFMA convolution kernel (roofline) ---------
 * While enabled, every launch of the convolution kernel is bracketed by two hipEvents on its
 * stream and recorded.  dcx_profile_enable(1) clears the record list.  After the caller has
 * synchronised the stream(s), dcx_profile_fetch() returns up to max_records records:
 * kernel_ids[i] (index into the instantiation table, see dcx_profile_kernel_name), n_images[i]
 * (images the grid covered), limited[i] (1 if a device-side patch count may have skipped some
 * of them), flops_per_image[i] = 2*cout*cin*ks*ks*Ho*Wo (algorithmic, un-padded), ms[i].
 * Ho x Wo is the convolution's own output: after an up-sampling on the read, before a pooling in the epilogue.
 * What a call records, in launch order (tests/instrument_cases.py derives the list from the oracle's layers):
 *   dcx_infer_batch          100 (detector conv1a, n = batch), conv1b .. conv4b, convPa|convDa as ONE launch (cout = 512,
 *                            flops of both), 102 (tail: the 1x1 heads convPb / convDb + arg-max + compaction, n = batch); with a
 *                            refiner: 101 (RefineNet conv1a + patch gather), conv1b .. conv5b, convPa (its 1x1 convPb and the tile
 *                            arg-max run in the same launch and are not counted), 103 (finalize) -- all with n = pool, limited = 1
 *   dcx_detector_forward     100, conv1b .. conv4b, convPa|convDa, then convPb and convDb as 1x1 launches (Ho x Wo = 1 x cells)
 *   dcx_refiner_forward      101 (conv1a on caller patches), conv1b .. conv5b, convPa, 103; n = max_patches, limited = 1 iff
 *                            d_total is given
 * The ids >= 100 carry flops_per_image = 0: the two conv1a layers, the detector's 1x1 heads inside the tail and RefineNet's convPb
 * are in no record's flops (0.156 of the 26.816 GFLOP of a 320x240 frame with 16 corners).
 * dcx_profile_enable(1) starts a session: it clears the record list and the clock probes of every slot (a synchronous call: set-up
 * code, not for a timed region).  dcx_profile_enable(0) stops recording and keeps the session's records.                  */
int dcx_profile_enable(int enabled);
int dcx_profile_enabled(void);       /* 1 while per-launch profiling is on */
int dcx_profile_count(void);
/* restrict recording to one kernel id (-1 = all): keeps the event overhead out of a timed region */
int dcx_profile_filter(int kernel_id);
int dcx_profile_sample(int every);   /* bracket only every `every`-th matching launch (1 = all): the two hipEvent records of a
                                        bracket keep the GPU idle for ~11 us, which a throughput measurement should not pay on
                                        every launch; every <= 1 is 1).  The count of matching launches is restarted by THIS call
                                        alone -- dcx_profile_enable(1) does not restart it, and launches that match while
                                        profiling is on count whether or not they are recorded: the first matching launch after
                                        dcx_profile_sample() is recorded, then every `every`-th, across sessions */
int dcx_profile_fetch(int* kernel_ids, int* n_images, int* limited, double* flops_per_image, float* ms,
                      int max_records);
/* kernel_id < 100: the convolution instantiation table; 100..103: the pipeline's other launches (detector conv1a, RefineNet
 * conv1a + patch gather, detector tail, refine finalize), recorded with flops_per_image = 0 while no filter is set */
const char* dcx_profile_kernel_name(int kernel_id);
/* effective shader clock (GHz) seen by workgroup 0 of each recorded launch: s_memtime ticks per
 * s_memrealtime (100 MHz) tick between its first and last instruction.  Same order as _fetch.
 * Only workgroup 0 of a launch writes probes, and only the first 1,024 records of a session own a probe slot: ghz[i] is 0 for
 * every later record (complete otherwise), for the ids >= 100, and for a convolution whose workgroup 0 had no work item (a
 * device-side patch count of 0, or fewer than 8 items under the XCD-aware walk) -- a mean over a session's clocks must leave
 * the zeros out.  One table per process, allocated on the device of the first profiled launch.                       */
int dcx_profile_clocks(float* ghz, int max_records);
/* raw 64 probe words of one recorded launch (kernel-tuning aid): [0..3] start/end {s_memtime, s_memrealtime},
 * then for the first 20 units of workgroup 0: s_memtime before the unit barrier, after it, after the MFMA loop (the small-launch
 * kernels dcx_conv_wino2hs / wino2ps write words 0..3 only).  DCX_E_ARG: NULL, record outside [0, 1024), or no table yet
 * (nothing has been profiled in this process)                                                                       */
int dcx_profile_probe_words(int record, unsigned long long* out64);

#ifdef __cplusplus
}
#endif
#endif /* DEEPCHARUCO_AMD_H */
