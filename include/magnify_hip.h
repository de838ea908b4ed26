/*
 * magnify_hip.h -- C ABI of the MI355X (gfx950) marker-detection hot path.
 *
 * The reference (FordyceLab/magnify v0.12.5) is pure Python; its compiled work on
 * this path comes from OpenCV, numba-JIT helpers and NumPy.
 * There is no FFI in the reference: each entry point below replaces one of those
 * native call sites (cited as file:line relative to the reference root) and is
 * what a ctypes binding in the reference would call.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer owned by the caller (PyTorch-ROCm
 *     tensors in this repo); the library never allocates or frees device memory;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*) and is
 *     asynchronous with respect to the host;
 *   - return value: 0 = ok, MG_EINVAL = bad argument, MG_ELAUNCH = HIP launch error;
 *   - "plane" = one (channel, time) image of H x W pixels; kernels are batched over
 *     planes (gridDim.z / gridDim.y) and read per-plane counters from device memory
 *     so that no host round trip is needed between stages;
 *   - thread-safe as long as streams and buffers are distinct.
 */
#ifndef MAGNIFY_HIP_H
#define MAGNIFY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OK 0
#define MG_EINVAL (-1)
#define MG_ELAUNCH (-2)
#define MG_EIO (-3) /* mg_host_read_runs only */

/* element types of image/tile buffers */
#define MG_U8 0
#define MG_U16 1
#define MG_F32 2
#define MG_F64 3

/* value stored in the angle map for "not an edge pixel" (angles are in [-pi, pi]) */
#define MG_NO_EDGE 100.0f
/* score written for circles that the exact prefilter proved to be below min_roundness */
#define MG_SCORE_SKIPPED (-2.0f)

/* Walk caps.  Most launchers cap their grid and let the kernel stride over the rest; every such cap has a name here, next
 * to its entry's other constants (MG_<KERNEL>_WALK...: workgroups in all, ..._PER_PLANE and the like: along x for one
 * plane), and DESIGN.md, "Capped launches and who walks them twice", lists the loops and the tests that take them round.
 * A grid's y (and z) holds at most MG_WALK_MAX_Y workgroups: more planes than that are walked with a stride as well. */
#define MG_WALK_MAX_Y 65535
#define MG_ZERO_WALK 1024 /* the clearing of counters and tables before an entry's kernel (a grid-stride loop) */

/* Canny map values (OpenCV's): 0 weak candidate, 1 not an edge, 2 strong edge */

int mg_version(void);

/* ------------------------------------------------------------------------------------
 * Host-side tables (no GPU needed).  utils.py:433-465 circle_points,
 * utils.py:398-430 filled_circle_points, utils.py:38 cv.circle(thickness=-1).
 * ---------------------------------------------------------------------------------- */

/* Perimeter offsets (row, col) in the reference's emission order.  Returns the number
 * of points (writes at most cap of them; pass cap=0 to query). */
int mg_circle_points(int r, int four_connected, int32_t* out_rc, int cap);
/* Filled disk of filled_circle_points(r) as per-row half widths: out[dy + r] = max |dx|
 * for dy in [-r, r].  r >= 2 (undefined below that in the reference).  Returns 2r+1. */
int mg_disk_halfwidths(int r, int32_t* out);
/* Filled disk of cv.circle(..., thickness=-1): out[|dy|] = max |dx|, |dy| in [0, r]. */
int mg_cv_disk_halfwidths(int r, int32_t* out);
/* Concatenated perimeter tables for radii min_r..max_r: offsets (row, col) int32,
 * expected angle atan2(row, col) float64 (utils.py:234), starts[nr+1].  Returns the
 * total number of points, or the required capacity if cap is too small. */
int mg_perimeter_table(int min_r, int max_r, int32_t* out_rc, double* out_expected, int32_t* out_starts, int cap);

/* ------------------------------------------------------------------------------------
 * A2 flat-field (preprocess.py:83-87) and A1 stitch (stitch.py:22-39)
 * ---------------------------------------------------------------------------------- */

/* Pass 1: the two global maxima M1 = max(clip(x - dark, 0)) and M2 = max(clip(x - dark, 0) / flat)
 * (float64, NaN-propagating) of each of n_groups equal groups of tiles (n_groups = 1: the
 * reference's single-assay semantics, the maxima span the whole array; n_groups = number of
 * assays when every time slice is its own assay).  d_max2 is double[n_groups][2], pre-initialised
 * by the caller to -inf.  dark/flat: scalar when d_dark / d_flat is NULL, else a (ty, tx) image
 * of type dark_dtype / flat_dtype (MG_F32 or MG_F64) broadcast over tiles.
 * d_scratch (optional): mg_flatfield_max_scratch_floats(dtype, ty, tx) floats owned by the caller and filled by
 * mg_flatfield_bound for THIS flat image (float32, integer pixel type `dtype`; -1 / MG_EINVAL where there is no such
 * path: the tile size must be a multiple of 8 (16) pixels): a per-chunk bound an eighth (a sixteenth) of the image's
 * size.  With it the integer-pixel / float32-flat path touches the flat image itself only where a pixel can still raise
 * M2 (same result, less traffic); the bound is computed once per flat image, not once per call. */
#define MG_FLATFIELD_MAX_WALK 4096          /* mg_flatfield_max: workgroups over all groups ... */
#define MG_FLATFIELD_MAX_WALK_PER_GROUP 512 /* ... and at most this many per group, on every path but the lean one */
#define MG_FLATFIELD_MAX_INT_WALK 2048      /* its scalar-operand integer path: workgroups over all groups ... */
#define MG_FLATFIELD_MAX_INT_WALK_MIN 64    /* ... and at least this many per group (below MG_FLATFIELD_MAX_WALK_PER_GROUP) */
#define MG_FLATFIELD_MAX_LEAN_WALK 1536 /* its integer-pixel / float32-flat path with the bound: one resident round */
#define MG_FLATFIELD_BOUND_WALK 2048   /* mg_flatfield_bound */
int64_t mg_flatfield_max_scratch_floats(int dtype, int ty, int tx);
int mg_flatfield_bound(const void* d_flat, int flat_dtype, int dtype, int ty, int tx, float* d_scratch,
                       int64_t scratch_floats, void* stream);
int mg_flatfield_max(const void* d_tiles, int dtype, int64_t n_tiles, int n_groups, int ty, int tx,
                     double dark, const void* d_dark, int dark_dtype,
                     double flat, const void* d_flat, int flat_dtype,
                     double* d_max2, float* d_scratch, int64_t scratch_floats, void* stream);

/* 1 when the correction is the identity for this pixel type: integer pixels, scalar dark 0 and scalar flat 1 (the
 * defaults of the reference's flatfield_correct, preprocess.py:62).  mg_flatfield_apply_stitch then only crops and
 * copies, and pass 1 (mg_flatfield_max) is not needed. */
int mg_flatfield_is_identity(int dtype, double dark, const void* d_dark, double flat, const void* d_flat);

/* Pass 2, fused with the stitch crop/concat: out[p, R*hy, Cc*hx] in the input dtype,
 * value = trunc(((clip(x - dark, 0) / flat) * M1) / M2) with M1, M2 = d_max2[p / planes_per_group].
 * Tiles are laid out (plane, tile_row, tile_col, ty, tx); hy = ty - overlap etc.
 * If apply_flatfield == 0 this is the pure stitch copy (any dtype, d_max2 unused).
 * d_minmax (optional, double[n_planes][2] pre-initialised to {+inf, -inf}) receives the
 * per-plane min/max of the values written (feeds to_uint8, utils.py:24-26). */
#define MG_STITCH_WALK_FILL 2048      /* the stitch passes: rows per row group are halved (32 .. 2) below this many workgroups */
#define MG_STITCH_WALK_PER_GROUP 1024 /* and with fewer than 32 rows at most this many workgroups walk a plane group's row groups */
int mg_flatfield_apply_stitch(const void* d_tiles, int dtype, int64_t n_planes, int n_tile_rows, int n_tile_cols,
                              int ty, int tx, int overlap, int apply_flatfield, int planes_per_group,
                              double dark, const void* d_dark, int dark_dtype,
                              double flat, const void* d_flat, int flat_dtype,
                              const double* d_max2, void* d_image, double* d_minmax, void* stream);

/* Pass 2 for a selection of planes: as mg_flatfield_apply_stitch with apply_flatfield = 1, but only the planes c of
 * every group of planes_per_group (<= 31) planes whose bit c is set in plane_mask are corrected -- written to their
 * usual place in d_image, their rows of d_minmax updated; the other planes and rows are left untouched.  n_planes (all
 * planes, a multiple of planes_per_group) and the layouts are those of the full pass; a later call with the
 * complementary mask completes the image block to what the full pass writes. */
int mg_flatfield_apply_stitch_planes(const void* d_tiles, int dtype, int64_t n_planes, int n_tile_rows, int n_tile_cols,
                                     int ty, int tx, int overlap, int planes_per_group, int plane_mask,
                                     double dark, const void* d_dark, int dark_dtype,
                                     double flat, const void* d_flat, int flat_dtype,
                                     const double* d_max2, void* d_image, double* d_minmax, void* stream);

/* Pass 2 with linear overlap blending of the tile seams: the operands, layouts and the image shape of
 * mg_flatfield_apply_stitch.  Inside the band of `overlap` pixels around every inner seam a pixel is the linear mix of
 * the values the plain pass would write for the two tiles that cover it (four where a row band and a column band
 * cross): position k of a band weighs the later tile (k + 0.5) / overlap.  Integer pixels: (sum of ny nx value +
 * D / 2) / D with D = (2 overlap)^2 in 64-bit integers; float pixels: float64, x first, then y, then the cast.  Outer
 * borders stay cropped.  d_minmax receives the min/max of the BLENDED values.  MG_EINVAL also for
 * 2 * overlap > min(ty, tx): a pixel would lie in two bands of one axis. */
int mg_flatfield_apply_stitch_blend(const void* d_tiles, int dtype, int64_t n_planes, int n_tile_rows, int n_tile_cols,
                                    int ty, int tx, int overlap, int apply_flatfield, int planes_per_group,
                                    double dark, const void* d_dark, int dark_dtype,
                                    double flat, const void* d_flat, int flat_dtype,
                                    const double* d_max2, void* d_image, double* d_minmax, void* stream);

/* Pass 2 on tiles moved by one integer shift each (tile registration): the operands, layouts and the image
 * of mg_flatfield_apply_stitch (blend = 0) or mg_flatfield_apply_stitch_blend (blend = 1) applied to
 *   tile'[r, c][y, x] = value[r, c][clamp(y - ey, 0, ty - 1), clamp(x - ex, 0, tx - 1)],
 * value: what the plain pass writes for that pixel of the tile, (ey, ex) = d_shift[table][r][c] (device int32,
 * (n_tables, n_tile_rows, n_tile_cols, 2)); the table of plane p is 0 when n_tables == 1, else p % n_time
 * (n_tables == n_time: one table per timepoint of (channel, time) planes).  d_minmax as there.  The tables are read
 * back and checked before the launch: the call copies them to the host and waits for the stream, so it must not be
 * made while the stream is being captured into a graph (the kernel itself clamps every read into the tile, so no table
 * can make it read out of bounds).  MG_EINVAL for an entry outside
 * [-overlap / 2, overlap / 2], for n_tables not in {1, n_time}, for blend not in {0, 1}, and for what the plain
 * (blend = 0) or the blended (blend = 1) entry refuses. */
int mg_flatfield_apply_stitch_shift(const void* d_tiles, int dtype, int64_t n_planes, int n_tile_rows, int n_tile_cols,
                                    int ty, int tx, int overlap, int apply_flatfield, int planes_per_group,
                                    double dark, const void* d_dark, int dark_dtype,
                                    double flat, const void* d_flat, int flat_dtype,
                                    const double* d_max2, void* d_image, double* d_minmax,
                                    const int32_t* d_shift, int n_tables, int n_time, int blend, void* stream);

/* ------------------------------------------------------------------------------------
 * Tile registration: the sums of the zero-mean normalised cross-correlation of every seam's overlap strips
 * ---------------------------------------------------------------------------------- */

/* d_planes: (n_planes, n_tile_rows, n_tile_cols, ty, tx) of `dtype`.  Seams in this order: (r, c) | (r, c + 1) at
 * index r (n_tile_cols - 1) + c, then (r, c) | (r + 1, c) at n_tile_rows (n_tile_cols - 1) + r n_tile_cols + c; A is
 * the first tile of the pair, B the second.  With v = overlap, m = max_shift the patch of B is q in
 * [m, ty - m) x [m, v - m) with offset o = (0, tx - v) for the first kind and [m, v - m) x [m, tx - m) with
 * o = (ty - v, 0) for the second; B[q] meets A[q + o + delta] for delta in [-m, m]^2.
 *   d_fixed (n_planes, n_seams, 3): n, sum B, sum B^2;
 *   d_sums  (n_planes, n_seams, 2m + 1, 2m + 1, 3): sum A, sum A^2, sum A B at [delta_y + m][delta_x + m];
 * int64 (exact) for MG_U8 / MG_U16, float64 for MG_F32 / MG_F64 -- the same bits on every run (partial sums per strip
 * in d_scratch, added in strip order; no atomics).  d_scratch: mg_seam_sums_scratch_bytes(...) bytes, 8-byte aligned.
 * MG_EINVAL / -1: max_shift < 1, 4 max_shift > overlap, max_shift > 32, overlap > min(ty, tx), more than 65535
 * planes or seams, a null pointer or too little scratch.  A 1 x 1 grid has no seams: MG_OK, nothing written. */
int64_t mg_seam_sums_scratch_bytes(int64_t n_planes, int n_tile_rows, int n_tile_cols, int ty, int tx, int overlap,
                                   int max_shift);
int mg_seam_sums(const void* d_planes, int dtype, int64_t n_planes, int n_tile_rows, int n_tile_cols, int ty, int tx,
                 int overlap, int max_shift, void* d_sums, void* d_fixed, void* d_scratch, int64_t scratch_bytes,
                 void* stream);

/* ------------------------------------------------------------------------------------
 * find_beads: following beads through time (find.py:564-602 cuts every timepoint's ROI at the time-0 position,
 * find.py:564: "TODO: Don't assume beads don't move across timesteps")
 * ---------------------------------------------------------------------------------- */

/* d_planes: the n_t planes (h, w) of ONE channel, plane t at d_planes + t * plane_stride elements of `dtype`.
 * d_beads (m, 3): row, col, r.  With md = max_drift, W = 2 md + 1, per bead g and timepoint t:
 *   patch: the pixels (y, x) with |y - row| <= half, |x - col| <= half, md <= y < h - md, md <= x < w - md (n of
 *   them, possibly none); B = plane[t_ref] on the patch, A(y, x) = plane[t][y + dy, x + dx] for (dy, dx) in [-md, md]^2;
 *   d_fixed (m, 3), optional: n, sum B, sum B^2;
 *   d_sums (m, n_t, W, W, 3), optional: sum A, sum A^2, sum A B at [dy + md][dx + md] (row t_ref: A = B's plane);
 *   int64 (exact) for MG_U8 / MG_U16, float64 for MG_F32 / MG_F64, the same bits on every call (no atomics);
 *   z = (n sAB - sA sB) / sqrt((n sAA - sA^2) (n sBB - sB^2)) in float64, each operation rounded on its own, IEEE
 *   division and square root; 0 where a variance term is <= 0 or z is not finite;
 *   d_shift (m, n_t, 2), d_score (m, n_t): the (dy, dx) of the largest z -- ties to the smallest dy^2 + dx^2, then
 *   the smallest dy, then the smallest dx -- and that z; row t_ref: (0, 0) and 1.0.
 * MG_EINVAL unless 1 <= max_drift <= 16, 1 <= half, 2 half + 1 <= 95, 2 half + 1 + 2 max_drift <= 127,
 * 0 <= t_ref < n_t, h, w > 0 (and m >= 0, m n_t < 2^31, no null pointer among planes, beads, shift, score); nothing
 * is launched then.  m == 0: MG_OK, nothing to write.  One kernel launch; no allocation, no synchronisation. */
int mg_track_beads(const void* d_planes, int dtype, int n_t, int64_t plane_stride, int h, int w, int t_ref,
                   const int32_t* d_beads, int m, int half, int max_drift, int32_t* d_shift, double* d_score,
                   void* d_sums, void* d_fixed, void* stream);

/* mg_track_beads around a per-timepoint base offset (find_beads(track="ncc", stage_drift=D): the stage moved, every
 * bead of timepoint t with it).  d_base (n_t, 2): (by, bx) of every timepoint; row t_ref ignores its base.  The
 * contract of mg_track_beads holds with these differences:
 *   patch of (g, t): the pixels (y, x) with |y - row| <= half, |x - col| <= half, 0 <= y < h, 0 <= x < w,
 *   md <= y + by < h - md, md <= x + bx < w - md -- the template and every displaced read inside the image; n now
 *   depends on t.  The geometry is made in 64 bits: a base far outside the image gives an empty patch;
 *   A(y, x) = plane[t][y + by + dy, x + bx + dx] for (dy, dx) in [-md, md]^2;
 *   d_fixed (m, n_t, 3), optional: n, sum B, sum B^2 of the patch of (g, t); d_sums as for mg_track_beads;
 *   d_shift[g, t] = (by + dy, bx + dx), the total displacement (the tie-breaks are on (dy, dx)); row t_ref: (0, 0)
 *   and 1.0; an empty patch: (0, 0) and 0.
 * With an all-zero base d_shift, d_score and d_sums equal those of mg_track_beads bit for bit and d_fixed[g, t] its
 * d_fixed[g] for every t.  MG_EINVAL where mg_track_beads returns it, and for a null d_base; nothing is launched then.
 * One kernel launch; no allocation, no synchronisation. */
int mg_track_beads_based(const void* d_planes, int dtype, int n_t, int64_t plane_stride, int h, int w, int t_ref,
                         const int32_t* d_beads, int m, int half, int max_drift, const int32_t* d_base,
                         int32_t* d_shift, double* d_score, void* d_sums, void* d_fixed, void* stream);

/* Binned planes (the coarse view of find_beads(stage_drift=D)).  d_planes: n_t planes (h, w) of `dtype`, plane t at
 * d_planes + t * plane_stride elements.  d_out (n_t, hb, wb) contiguous float32, hb = h / bin, wb = w / bin:
 * out[t, i, j] = the sum of the bin x bin block at (bin i, bin j) of plane t; the trailing h % bin rows and w % bin
 * columns are not read.  MG_U8 / MG_U16: exact (64 * 65535 < 2^24).  MG_F32 / MG_F64: summed in float64 -- the
 * block's rows from the top, each from the left -- and rounded to float32 once: the same bits on every call.  No
 * atomics.  MG_EINVAL, with nothing launched: bin not in {2, 4, 8}, h < bin, w < bin, n_t < 1, an unknown dtype, a
 * null pointer.  One kernel launch; no allocation, no synchronisation. */
#define MG_BIN_WALK 2048 /* workgroups of 256 items (a run of output columns of one output row) */
int mg_bin_planes(const void* d_planes, int dtype, int n_t, int64_t plane_stride, int h, int w, int bin,
                  float* d_out, void* stream);

/* Per-plane min/max (utils.py:24-25) of strided planes.  d_minmax double[n_planes][2],
 * pre-initialised to {+inf, -inf}.  Strides are in elements. */
#define MG_PLANE_MINMAX_WALK 1024 /* workgroups per plane */
int mg_plane_minmax(const void* d_src, int dtype, int n_planes, int64_t plane_stride, int h, int w,
                    int64_t row_stride, double* d_minmax, void* stream);

/* ------------------------------------------------------------------------------------
 * rotate (preprocess.py:54-59; the disabled body there: dask_image.ndinterp.rotate(order=1, reshape=False))
 * ---------------------------------------------------------------------------------- */

/* Bilinear 2 x 2 affine resampling of n_planes contiguous (h, w) planes of `dtype`, d_src -> d_dst (distinct buffers
 * of the same size and type), with the semantics of scipy.ndimage.affine_transform(order=1, mode="constant", cval=0):
 * `matrix` (4 doubles, row-major) and `offset` (2 doubles) are HOST pointers, read before the call returns.  All
 * arithmetic is float64, every operation rounded on its own (no fused multiply-add), in this order, for output pixel
 * (oy, ox):
 *   cy = (offset[0] + oy * matrix[0]) + ox * matrix[1],  cx = (offset[1] + oy * matrix[2]) + ox * matrix[3];
 *   cy < 0, cy > h - 1, cx < 0 or cx > w - 1: the value is 0 (no interpolation across the border); otherwise
 *   fy = floor(cy), ty = cy - fy, y0 = fy, y1 = min(y0 + 1, h - 1), and the same for x;
 *   v = (((p00 * (1 - ty)) * (1 - tx) + (p01 * (1 - ty)) * tx) + (p10 * ty) * (1 - tx)) + (p11 * ty) * tx;
 *   written as floor(v + 0.5) for MG_U8 / MG_U16, (float)v for MG_F32, v for MG_F64.
 * d_minmax (optional, double[n_planes][2] pre-initialised to {+inf, -inf}) receives the per-plane min/max of the
 * values written, as for mg_flatfield_apply_stitch.  MG_EINVAL: a null or misaligned pointer, d_src == d_dst, a
 * negative size, an unknown dtype, a non-finite matrix or offset; MG_OK without a launch when there is no pixel. */
#define MG_ROTATE_WALK 2048 /* workgroups over all planes; each walks its share of a plane's tiles */
int mg_affine_bilinear(const void* d_src, void* d_dst, int dtype, int64_t n_planes, int h, int w,
                       const double* matrix, const double* offset, double* d_minmax, void* stream);

/* ------------------------------------------------------------------------------------
 * Shading model (BaSiC, Peng et al. 2017): fit of a flat- and a dark-field from training tiles and its apply fused
 * with the stitch crop (DESIGN.md §4 "shading"; oracle tests/ref_shading.py).  The fit's state lives in one device
 * workspace of mg_shading_workspace_bytes(n, w) bytes (n images, w x w working grid, 1 <= w <= 128), 256-byte aligned;
 * mg_shading_offset(n, w, field) is the byte offset of region `field`:
 *   0 D, 1 E, 2 Y, 3 weight (float32 n x w^2); 4 W_hat, 5 F_w, 6 A_off, 7 M (scratch; mean_n XA before
 *   mg_shading_reweight), 8 T (scratch), 9 mean over images of D, 10 min over images of D (float64 w^2);
 *   11 DCT-II table C[k][x], 12 its transpose (float64 w^2); 13 coeff (float64 n); 14-16 partial sums (internal);
 *   17 Gram matrix D D^T (float64 n x n); 18 scalars (float64 x 32); 19 flags (int32 x 8).
 * Scalars: 0 mu, 1 mu_bar, 2 lambda_f, 3 lambda_d, 4 tol, 5 ||D||_F, 6 b_up (min of D), 7 B1_offset, 8 mean(F_w),
 *   9 mean(A), 10 cbar (mean coeff of the images with coeff < 1), 11 mean(A1), 12 the stop ratio ||Z||_F / ||D||_F;
 *   8-12 are those of the last iteration, 7, 10 and 11 of the last one whose darkfield step ran.
 * Flags: 0 done, 1 ALM iterations of the pass, 2 max iterations, 3 skip-dark (no darkfield asked for, or no image with
 *   coeff < 1 in the last iteration: its darkfield step was skipped).
 * Region 14, the per-image totals of the last iteration (float64 n x 8): 0 sum of R = D - E, 1 the same over the
 *   pixels with F_w > mean(F_w) - 1e-6 ("hi"), 2 over those with F_w < mean(F_w) + 1e-6 ("lo"), 3 sum of A,
 *   4 sum of Z^2, 5 count of hi pixels, 6 count of lo pixels, 7 B1c = (R hi / count hi - R lo / count lo) / mean(A).
 *   After a darkfield iteration region 7 (M) holds the shrunk DCT of the darkfield residual, otherwise the mean
 *   over images of D - A - E + Y / mu.
 * -1 / MG_EINVAL for a bad argument.
 * ---------------------------------------------------------------------------------- */
int64_t mg_shading_workspace_bytes(int n, int w);
int64_t mg_shading_offset(int n, int w, int field);
/* Area downsample of n (ty, tx) tiles of `dtype` (ty, tx >= w) to d_out[n][w][w] float32, float64 accumulation. */
int mg_shading_downsample(const void* d_tiles, int dtype, int64_t n, int ty, int tx, int w, float* d_out, void* stream);
/* From D in the workspace: DCT tables, per-pixel mean / min over images, Gram matrix, weight = 1. */
int mg_shading_prepare(void* d_ws, int n, int w, void* stream);
/* d_out = dct2(d_in) (inverse = 0) or idct2(d_in) (inverse = 1), orthonormal, float64 w x w; needs mg_shading_prepare. */
int mg_shading_dct2(void* d_ws, int n, int w, const double* d_in, double* d_out, int inverse, void* stream);
/* Fresh ALM state of one reweighting pass (mu_bar = 1e7 mu, rho = 1.5, ent1 = 1, ent2 = 10). */
int mg_shading_alm_begin(void* d_ws, int n, int w, int get_darkfield, int max_iterations, double mu, double lam_f,
                         double lam_d, double tol, double norm_f, double b_up, void* stream);
/* Enqueue k ALM iterations; once the stop test holds or max_iterations is reached the `done` flag is set and the
 * remaining iterations return at once.  No host synchronisation. */
int mg_shading_alm_iterate(void* d_ws, int n, int w, int k, int get_darkfield, void* stream);
/* weight = 1 / (|E / M| + epsilon), scaled to mean 1 (M: mean_n XA, written by the caller). */
int mg_shading_reweight(void* d_ws, int n, int w, double epsilon, void* stream);
/* Bilinear upsample (half-pixel centres, clamped) of the w x w float64 fields to ty x tx float32; the flat is divided
 * by its float64 mean.  d_partial: 256 float64 of scratch. */
int mg_shading_upsample(const double* d_flat_w, const double* d_dark_w, int w, int ty, int tx, double* d_partial,
                        float* d_flat, float* d_dark, void* stream);
/* out = (x - dark) / flat fused with the stitch crop / concat (as mg_flatfield_apply_stitch): tiles (n_fields *
 * planes_per_field planes, n_tile_rows, n_tile_cols, ty, tx) of `dtype`; plane p uses field p / planes_per_field of
 * d_flat / d_dark (float32, stride ty * tx).  u8 / u16 / f32 tiles in float32, f64 in float64; integer outputs
 * clamped to [0, max] and truncated.  d_minmax (optional, double[planes][2] pre-set to {+inf, -inf}): per-plane
 * min / max of the values written. */
#define MG_SHADING_APPLY_WALK 2048 /* workgroups in all; each walks its share of the row groups */
#define MG_SHADING_SETUP_WALK 1024 /* k_setup of mg_shading_prepare, k_begin of mg_shading_alm_begin */
int mg_shading_apply_stitch(const void* d_tiles, int dtype, int n_fields, int64_t planes_per_field, int n_tile_rows,
                            int n_tile_cols, int ty, int tx, int overlap, const float* d_flat, const float* d_dark,
                            void* d_image, double* d_minmax, void* stream);
/* mg_shading_apply_stitch with the seams blended as in mg_flatfield_apply_stitch_blend (the values mixed are those
 * mg_shading_apply_stitch writes). */
int mg_shading_apply_stitch_blend(const void* d_tiles, int dtype, int n_fields, int64_t planes_per_field,
                                  int n_tile_rows, int n_tile_cols, int ty, int tx, int overlap, const float* d_flat,
                                  const float* d_dark, void* d_image, double* d_minmax, void* stream);

/* mg_shading_apply_stitch on tiles moved by one integer shift each, blended or not: the shift arguments and their
 * checks are those of mg_flatfield_apply_stitch_shift (planes: n_fields * planes_per_field). */
int mg_shading_apply_stitch_shift(const void* d_tiles, int dtype, int n_fields, int64_t planes_per_field,
                                  int n_tile_rows, int n_tile_cols, int ty, int tx, int overlap, const float* d_flat,
                                  const float* d_dark, void* d_image, double* d_minmax, const int32_t* d_shift,
                                  int n_tables, int n_time, int blend, void* stream);

/* ------------------------------------------------------------------------------------
 * A3-A6 edge stage of find_circles (utils.py:20-27, 115-142)
 * ---------------------------------------------------------------------------------- */

/* to_uint8 (global min/max rescale, truncating) fused with cv.GaussianBlur(5x5, sigma 0):
 * d_blur[n_planes][h][w] u8.  d_u8 (optional, same shape) receives the un-blurred uint8
 * image.  With dtype == MG_U8 and d_minmax == NULL the input is taken as already uint8. */
int mg_to_uint8_blur(const void* d_src, int dtype, int n_planes, int64_t plane_stride, int h, int w,
                     int64_t row_stride, const double* d_minmax, uint8_t* d_blur, uint8_t* d_u8, void* stream);

/* Scharr gradients of the blurred image and a histogram of the integer squared
 * magnitude m = dx^2 + dy^2 (the float32 gradient of utils.py:120 is sqrt(float(m)), a
 * monotone function of m, so np.quantile's order statistics are recovered exactly).
 * mode 0 (combined, 12288 bins per plane): bins [0, 8192) count m exactly, bin 8192 + (m >> 13)
 *   counts the rest coarsely -- one pass suffices whenever both quantile ranks fall below 8192;
 * mode 1 (window, 8192 bins per plane): bin m - d_base[plane] for m in [base, base + 8192); a plane whose base
 *   is 0xFFFFFFFF is skipped.
 * d_hist must be pre-zeroed. */
int mg_scharr_hist(const uint8_t* d_blur, int n_planes, int h, int w, int mode, const uint32_t* d_base,
                   uint32_t* d_hist, uint32_t* d_scratch, int64_t scratch_words, void* stream);
/* Words of caller-owned scratch that let mg_scharr_hist hand its per-workgroup histograms over with
 * plain stores (summed by a second small kernel) instead of one global atomicAdd per non-empty bin.
 * d_scratch == NULL selects the atomic hand-over. */
int64_t mg_scharr_hist_scratch_words(int n_planes, int h, int w, int mode);

/* mg_to_uint8_blur and mg_scharr_hist (mode 0) of the same planes as ONE call (utils.py:20-27 and 115-125 follow each
 * other in find_circles): where the input is an integer type, no un-blurred copy is asked for, w % 4 == 0 and the
 * rows are aligned, one kernel blurs a strip and histograms its Scharr magnitudes while the blurred rows are still
 * in registers; otherwise the two passes run one after the other.  Same results either way.  d_hist must be
 * pre-zeroed; d_scratch: mg_blur_hist_scratch_words words (NULL: the two passes, histogram handed over by atomics). */
int mg_to_uint8_blur_hist(const void* d_src, int dtype, int n_planes, int64_t plane_stride, int h, int w,
                          int64_t row_stride, const double* d_minmax, uint8_t* d_blur, uint8_t* d_u8, uint32_t* d_hist,
                          uint32_t* d_scratch, int64_t scratch_words, void* stream);
int64_t mg_blur_hist_scratch_words(int n_planes, int h, int w);

/* np.quantile(grad, q) for the two Canny quantiles and cv::Canny's threshold preparation (utils.py:126-134),
 * from the combined histogram of mg_scharr_hist (mode 0), on the device: ranks4 (HOST array) = the prev / next
 * order-statistic indices of numpy's linear interpolation for the low and the high quantile, gamma_* its
 * float32 weights (magnify_amd.hotpath.quantile_indexes).  Outputs d_thresh[n_planes][2] (the integer
 * thresholds mg_canny_nms takes), d_quantiles[n_planes][2] (float32, what np.quantile returns) and
 * d_unresolved[n_planes]: low byte = the number of WINDOW passes the plane still needs (0: thresholds valid) -- one
 * per distinct coarse bin that one of its ranks fell into --, next byte = the number it needs in all.  With d_state (int32 [n_planes][16]) and d_win_base
 * (uint32 [n_planes]) the passes stay on the device: d_win_base receives the base of pass 0 (0xFFFFFFFF: the plane
 * needs none and mg_scharr_hist mode 1 skips it); then, for pass = 0, 1, ...: clear d_hist_win
 * [n_planes][8192], mg_scharr_hist(mode 1, d_base = d_win_base, d_hist = d_hist_win),
 * mg_edge_thresholds_window(pass) -- which resolves the ranks of that window, writes the next base and, after a
 * plane's last window, its thresholds and d_unresolved = 0.  At most 4 passes.  Both NULL: detection only. */
int mg_edge_thresholds(const uint32_t* d_hist, int n_planes, const int64_t* ranks4, float gamma_low, float gamma_high,
                       int32_t* d_thresh, float* d_quantiles, int32_t* d_unresolved, int32_t* d_state,
                       uint32_t* d_win_base, void* stream);
int mg_edge_thresholds_window(const uint32_t* d_hist_win, int n_planes, int pass, float gamma_low, float gamma_high,
                              int32_t* d_state, uint32_t* d_win_base, int32_t* d_thresh, float* d_quantiles,
                              int32_t* d_unresolved, void* stream);

/* Bitmaps over pixels use the linear layout bit i of word k <-> pixel 32 k + i (i = y * w + x);
 * words_per_plane >= ceil(h w / 32) + 1. */

/* cv.Canny(dx, dy, L2gradient=True) non-maximum suppression + double threshold with the
 * already prepared integer thresholds d_thresh[n_planes][2] = {low, high}.  Output: two bitmaps,
 * d_weak (local maxima with m > low: OpenCV map values 0 and 2) and d_strong (m > high: value 2).
 * d_class (optional, [n_planes][3][words_per_plane]): bit planes c0, c1, c2 of every pixel's gradient
 * orientation bin floor((atan2(dy, dx) mod pi) / (pi / 8)) = 4 c1 + 2 c0 + c2, decided exactly on the integer
 * Scharr gradient: the quarter 2 c1 + c0 (same sign: |dy| < |dx| -> 0 else 1; opposite sign: |dy| > |dx| -> 2
 * else 3) and its upper half c2 (tan(pi/8) = sqrt(2) - 1 and tan(3 pi/8) = sqrt(2) + 1 as integer
 * inequalities (|dx| + |dy|)^2 > 2 dx^2, (|dy| - |dx|)^2 > 2 dx^2); consumed by the scoring prefilters
 * (mg_score_circles: quarters; mg_score_circles_keyed: eighths).
 * The words behind the last pixel of a plane are never written: the caller zeroes the bitmaps once, when it
 * allocates them (the words inside the image are overwritten by every call). */
int mg_canny_nms(const uint8_t* d_blur, int n_planes, int h, int w, const int32_t* d_thresh, uint32_t* d_weak,
                 uint32_t* d_strong, uint32_t* d_class, int64_t words_per_plane, void* stream);
/* How mg_canny_nms cuts an (aligned) image of width w: columns per wave strip, rows per wave, rows per workgroup. */
int mg_canny_nms_strips(int w, int* strip_w, int* wave_rows, int* group_rows);

/* One sweep of 8-connected hysteresis, bit-parallel on the bitmaps: every 256 x 256 tile grows its strong set into
 * its weak set to a fixed point in LDS (halo from global memory) and ORs the new bits into d_strong.  Where that
 * growth reaches a weak, not yet strong pixel of a NEIGHBOURING tile, the neighbour's flag in d_flags_out
 * (uint8[n_planes][tiles_y][tiles_x], mg_hysteresis_tiles; pre-zeroed) is set and d_changed[n_planes] becomes
 * non-zero for the plane: another sweep is needed, in which only the flagged tiles (d_flags_in = that d_flags_out)
 * are worked on.  Call until a sweep leaves d_changed at zero: d_strong is then the edge map of utils.py:142.
 * d_flags_in = NULL (first sweep, or a caller without flags): every tile is worked on. */
int mg_canny_hysteresis(const uint32_t* d_weak, uint32_t* d_strong, int64_t words_per_plane, int n_planes, int h,
                        int w, uint32_t* d_changed, const uint8_t* d_flags_in, uint8_t* d_flags_out, void* stream);
int mg_hysteresis_tiles(int h, int w, int* tiles_x, int* tiles_y);

/* Inspection helper: bitmap -> {0,1} bytes, d_out[n_planes][n_bits]. */
#define MG_UNPACK_BITS_WALK 4096 /* workgroups per plane */
int mg_unpack_bits(const uint32_t* d_bits, int64_t words_per_plane, int n_planes, int64_t n_bits, uint8_t* d_out,
                   void* stream);

/* grid_array (utils.py:347-377) from the bitmap.  phases & 1: d_cell_counts / d_cell_starts [n_planes][gr*gc]
 * (gr = ceil(h / grid), gc = ceil(w / grid)) and d_num_edges[n_planes]; phases & 2: the cell-major /
 * row-major-inside-cell list d_coords[n_planes][coord_cap][2] (row, col) is filled.  A caller without an estimate of
 * the edge count runs phase 1, reads d_num_edges and sizes the list; one with a capacity from an earlier call runs
 * both at once (phases = 3): a plane with more edges than coord_cap then gets d_num_edges = 0 -- nothing downstream
 * indexes beyond the list -- and its true count in d_edge_totals[n_planes] (optional), for the caller to check when it
 * next synchronises.  d_scan_state (optional): mg_edge_grid_scan_words(...) 64-bit words owned by the caller
 * (cleared by the call itself): the prefix sum over the cells then runs on many workgroups per plane, chunk totals
 * handed on through these words, chunks taken by ticket (no assumption about the order workgroups are dispatched in). */
int64_t mg_edge_grid_scan_words(int n_planes, int h, int w, int grid);
int mg_edge_grid(const uint32_t* d_edge_bits, int64_t words_per_plane, int n_planes, int h, int w, int grid,
                 int32_t* d_cell_counts, int32_t* d_cell_starts, int32_t* d_num_edges, int32_t* d_coords,
                 int64_t coord_cap, uint64_t* d_scan_state, int32_t* d_edge_totals, int phases, void* stream);

/* float32 gradient angle arctan2(dy, dx) (utils.py:118-119, 170) at every edge pixel of the
 * compact list, evaluated in float64 and rounded once: d_angle[n_planes][h][w] is written at
 * edge pixels only. */
#define MG_EDGE_ANGLES_WALK 1048576 /* workgroups per plane: one edge per thread up to here */
int mg_edge_angles(const uint8_t* d_blur, int n_planes, int h, int w, const int32_t* d_coords, int64_t coord_cap,
                   const int32_t* d_num_edges, float* d_angle, void* stream);

/* ------------------------------------------------------------------------------------
 * A8-A11 RANSAC circle candidates, scoring, greedy NMS (utils.py:145-199, 225-344)
 * ---------------------------------------------------------------------------------- */

/* Layout of the circle de-duplication bitmap: centres are binned into 64 x 64 tiles of the padded
 * centre grid (row + max_r, col + max_r); every (tile, radius) pair owns one 4096-bit "layer"
 * (bit = (row_in_tile << 6) | col_in_tile); layers are ordered (tile_row, tile_col, r).
 * n_layers = tile_rows * tile_cols * (max_r - min_r + 1), bitmap_words = 128 * n_layers. */
int mg_dedup_layout(int h, int w, int min_r, int max_r, int* n_tile_rows, int* n_tile_cols, int64_t* n_layers,
                    int64_t* bitmap_words);

/* candidate_circles (utils.py:295-344) with the build's counter-based RNG (the reference
 * is unseeded): iteration i of plane p draws three 32-bit uniforms from
 * splitmix64(seed[p] + (3 i + k + 1) * golden) >> 32.  p0 is a jittered stratified draw: iteration i
 * owns the slice [a, b) = [floor(i E / K), floor((i + 1) E / K)) of the cell-major edge list and
 * takes p0 = coords[a + (u0 * max(b - a, 1) >> 32)] (every edge equally likely, consecutive
 * iterations spatially coherent); p1, p2 = p0's cell list[u * count >> 32].  Then steps 4 of filter_circles
 * (utils.py:157-166): radius window, round-half-even, off-image rejection.  Survivors set
 * their bit in d_bitmap[n_planes][bitmap_words] (mg_dedup_layout), which de-duplicates them:
 * a circle's score depends only on (row, col, r).
 * d_raw (optional, float32 [n_planes][num_iter][3]) receives the unfiltered circles. */
#define MG_CANDIDATES_WALK 2048     /* workgroups per plane of the general kernel */
#define MG_CANDIDATES_TAB_WALK 1024 /* of the table kernel: at most this many per plane ... */
#define MG_CANDIDATES_TAB_FILL 1024 /* ... and about this many over all planes at least */
#define MG_CANDIDATES_TAB_RUN 4     /* consecutive iterations a lane of the table kernel takes per trip */
int mg_candidate_circles(const int32_t* d_coords, int64_t coord_cap, const int32_t* d_cell_starts,
                         const int32_t* d_cell_counts, const int32_t* d_num_edges, int n_planes, int h, int w,
                         int grid, const uint64_t* d_seeds, int64_t num_iter, int min_r, int max_r,
                         uint32_t* d_bitmap, int64_t bitmap_words, float* d_raw, void* stream);

/* The same candidates WITHOUT global atomics: every iteration stores a 32-bit key into
 * d_keys[n_planes][num_iter] -- (tile << 17) | ((r - min_r) << 12) | ((pr & 63) << 6) | (pc & 63) with
 * (pr, pc) = (row + max_r, col + max_r), tile = (pr >> 6) * tile_cols + (pc >> 6) -- or 0xFFFFFFFF when
 * step 4 of filter_circles rejects it.  Needs tile_rows * tile_cols < 32768 and max_r - min_r < 32
 * (MG_EINVAL otherwise: use mg_candidate_circles). */
int mg_candidate_keys(const int32_t* d_coords, int64_t coord_cap, const int32_t* d_cell_starts,
                      const int32_t* d_cell_counts, const int32_t* d_num_edges, int n_planes, int h, int w, int grid,
                      const uint64_t* d_seeds, int64_t num_iter, int min_r, int max_r, uint32_t* d_keys, float* d_raw,
                      void* stream);

/* Keys -> unique keys, grouped by tile.  Because p0 is a stratified draw over the cell-major edge
 * list, the iterations that can place a centre in a given 64 x 64 tile form one contiguous key range
 * per cell row within max_r + 2 of the tile; one workgroup per pair of tiles scans them, ORs its own
 * keys into an LDS copy of the tiles' layers, counts, reserves its slice of the plane's list with one
 * atomicAdd on d_num_circles (zeroed by this call unless counters_clear, see below) and stores the unique keys of each tile in
 * (r, row, col) order:
 *   d_unique_keys[n_planes][circle_cap] uint32, d_tile_ranges[n_planes][n_tiles][2] int32 = (first, count)
 *   of every tile (n_tiles = tile rows x tile cols of mg_dedup_layout), d_num_circles[n_planes].
 * The slices of different workgroups land in arrival order: list positions are not canonical, the
 * keys are (mg_nms_rounds / mg_collect_circles take them as tie-breakers).  d_cell_* / d_num_edges /
 * grid / num_iter must be those the keys were generated with.
 * d_layer_starts (optional, [n_planes][n_tiles][nr + 1], nr = max_r - min_r + 1): list index of the first key
 * of every radius of every tile, entry nr = the tile's end (mg_score_circles_keyed deals its work by radius).
 * counters_clear (here and in mg_score_circles_keyed, mg_nms_rounds, mg_collect_circles): 0 -- the call clears the
 * per-plane counters it accumulates into (d_num_circles / d_num_surv / d_undecided / d_num_out) with a launch of its
 * own; 1 -- the caller has cleared them (a caller that keeps all its counters in one block clears it once per chain:
 * eight ~5 us launches fewer, a tenth of a single-plane call). */
int mg_keys_to_circles(const uint32_t* d_keys, int64_t num_iter, const int32_t* d_cell_starts,
                       const int32_t* d_cell_counts, const int32_t* d_num_edges, int n_planes, int h, int w, int grid,
                       int min_r, int max_r, uint32_t* d_unique_keys, int64_t circle_cap, int32_t* d_tile_ranges,
                       int32_t* d_num_circles, int32_t* d_layer_starts, int counters_clear, void* stream);

/* Ordered compaction of the bitmap into the unique circle list in the build's canonical order
 * (tile_row, tile_col, r, row, col): d_circles[n_planes][circle_cap][3] int32 (row, col, r),
 * d_num_circles[n_planes], and d_layer_offsets[n_planes][n_layers + 1] (start of every layer in
 * the list; the last entry is the total).  Clears the bitmap words it consumes (the bitmap is
 * all-zero again afterwards). */
int mg_bitmap_to_circles(uint32_t* d_bitmap, int64_t bitmap_words, int n_planes, int h, int w, int min_r,
                         int max_r, int32_t* d_layer_offsets, int32_t* d_circles, int64_t circle_cap,
                         int32_t* d_num_circles, void* stream);

/* mean_grad / len(perimeter) (utils.py:183-188, 225-251), one workgroup per centre tile with the
 * tile's window of the 1-bit edge map staged in LDS.
 * Pass A (exact prefilter): every term of the sum is <= 1, so circles with fewer than
 * min_roundness * P edge pixels on their perimeter cannot pass (they get MG_SCORE_SKIPPED when
 * write_skipped != 0, else their score is left unwritten).  With d_class_bits (optional, from
 * mg_canny_nms) an edge pixel only counts where its gradient orientation class is not the one
 * perpendicular to the perimeter point's radial direction: such a pixel is at least pi/4 away from
 * radial, its term 4 |d - pi/2| / pi - 1 is <= 0, and the bound stays exact.
 * Pass B: the reference's float64 sum, sequential in perimeter order, stored float32 and divided
 * by the perimeter length in float32; d_angle holds the gradient angle at edge pixels
 * (mg_edge_angles); per_total = number of entries of the perimeter tables.
 * Circles with score >= min_roundness (float32 compare, utils.py:191) are appended (unordered) to
 * d_alive[n_planes][circle_cap] (indices into d_circles), d_num_alive[n_planes] pre-zeroed;
 * d_max_rc[n_planes][2] (pre-set to INT32_MIN) receives max row / max col of the alive circles
 * (the claim-grid extent of utils.py:268-270).  d_num_scored (optional, [n_planes], pre-zeroed)
 * counts the circles that reached pass B.
 * Input, one of: (a) d_unique_keys + d_tile_ranges from mg_keys_to_circles (d_layer_offsets unused):
 * the circles are decoded from the keys and d_circles[n_planes][circle_cap][3] is an OUTPUT, written
 * only at the positions of the circles that pass the threshold (all that suppression and the ordered
 * output read); (b) d_unique_keys == NULL: d_circles + d_layer_offsets from mg_bitmap_to_circles.
 * dedup_centres != 0 (only when greedy suppression with min_dist > 0 follows): of the passing circles that
 * share a centre, only the first in suppression order (score desc, radius asc) is appended to d_alive --
 * the others have the same suppression ring and are rejected whatever happens to the first one
 * (utils.py:254-292), so the kept set is unchanged; best effort per tile (64 parked circles). */
#define MG_SCORE_EXACT_WALK 4096     /* the exact scoring pass: workgroups over all planes (16 .. 256 per plane) */
#define MG_SCORE_PREFILTER_WALK 4096 /* the prefilter: persistent workgroups that are dealt the super-tiles of all planes */
int mg_score_circles(const float* d_angle, const uint32_t* d_edge_bits, const uint32_t* d_class_bits,
                     int64_t words_per_plane, int n_planes, int h, int w, int32_t* d_circles, int64_t circle_cap,
                     const int32_t* d_layer_offsets, const uint32_t* d_unique_keys, const int32_t* d_tile_ranges,
                     int min_r, int max_r, const int32_t* d_per_rc, const double* d_per_expected,
                     const int32_t* d_per_starts, int per_total, float min_roundness, int write_skipped,
                     int dedup_centres, float* d_scores, int32_t* d_alive, int32_t* d_num_alive, int32_t* d_max_rc,
                     int32_t* d_num_scored, void* stream);

/* The keyed path's scoring (same scores and same passing set as mg_score_circles input (a), which remains for
 * radii outside mg_score_keyed_supported): two kernels.
 * Prefilter: a workgroup per super-tile of 2 x 4 centre tiles (128 x 256 positions) with the edge window in LDS as one byte per
 * pixel position (low nibble: the gradient-orientation bin of mg_canny_nms' class planes, 0xC = no edge; high nibble:
 * the same for the pixel to the right, so one byte read returns two adjacent perimeter points of a row); a lane per
 * circle, all circles of a wave of one radius, the perimeter walked as straight-line code per radius.  For every pair of
 * opposite perimeter points the two window nibbles select, in one byte permute, UPPER BOUNDS of the two pixels'
 * terms 4 |d - pi/2| / pi - 1 (utils.py:244-249) from the pair's table (mg_score_pair_table: the distance
 * between the points' radial direction and the pixel's orientation bin bounds the term); the bounds are summed
 * in 1/64 (rounded up) and a circle whose bound is below min_roundness * P - 1e-3 is dropped -- exact: every
 * term <= its bound.  Survivors are appended to d_surv_list[n_planes][surv_cap][2] (scratch: list index and key;
 * surv_cap >= circle_cap is required: it can then never overflow), d_num_surv[n_planes] (scratch, zeroed here).
 * Exact pass: the reference's float64 sum in perimeter order, 4 (16 at small batches) lanes per survivor (the edge
 * pixels on the perimeter and their angles are found in parallel, the terms added in order); the gradient angle of a
 * hit is d_angle's entry or, with d_angle == NULL, computed on demand from d_blur exactly as mg_edge_angles
 * does (so neither the angle map nor its pass is needed).  Outputs as mg_score_circles (no same-centre
 * reduction: the suppression treats same-centre circles correctly by itself); d_num_scored = survivors.
 * d_class_bits is required. */
int mg_score_keyed_supported(int min_r, int max_r); /* 1: 2 <= min_r, max_r <= 26 */
/* out_entries[27][80]: for radius r and pair k of opposite perimeter points, 8 signed bytes = bound (1/64) per
 * orientation bin.  Returns the number of entries (2160); fills them when cap >= that. */
int mg_score_pair_table(uint64_t* out_entries, int cap);
/* first point (dr, dc) of every pair of radius r, in table order; returns the number of pairs */
int mg_score_pairs(int r, int32_t* out_rc, int cap);
/* LDS byte reads of the prefilter's walk of radius r (two adjacent perimeter points of a row come with one read):
 * taken from the structure the kernel is instantiated from; 0 for r outside 2..26 */
int mg_score_walk_reads(int r);
int mg_score_circles_keyed(const uint8_t* d_blur, const float* d_angle, const uint32_t* d_edge_bits,
                           const uint32_t* d_class_bits, int64_t words_per_plane, int n_planes, int h, int w,
                           int32_t* d_circles, int64_t circle_cap, const uint32_t* d_unique_keys,
                           const int32_t* d_layer_starts, int min_r, int max_r, const int32_t* d_per_rc,
                           const double* d_per_expected, const int32_t* d_per_starts, int per_total,
                           const uint64_t* d_pair_table, float min_roundness, int write_skipped, float* d_scores,
                           int32_t* d_alive, int32_t* d_num_alive, int32_t* d_max_rc, int32_t* d_num_scored,
                           int32_t* d_surv_list, int64_t surv_cap, int32_t* d_num_surv, int counters_clear,
                           void* stream);

/* n_rounds rounds of the parallel-but-equivalent greedy suppression of filter_neighbors
 * (utils.py:254-292).  Priority = (score desc, tie key asc) -- the build's canonical tie order
 * (tile_row, tile_col, r, row, col): d_tie_keys[n_planes][circle_cap] (the unique keys of
 * mg_keys_to_circles) or, when NULL, the index in d_circles (canonical after mg_bitmap_to_circles).
 * d_grid[n_planes][grid_cap] uint64 claim grid pre-set to all-ones;
 * d_state[n_planes][circle_cap] uint8 (0 undecided, 1 kept, 2 dropped) pre-zeroed for
 * alive circles; round k sets d_undecided[k * undecided_stride + plane] to 0 (counters_clear: the caller has), or to
 * 1 when a circle of the plane is still undecided after it: the rounds have converged when a round leaves none.
 * Ring = 4-connected perimeter of radius min_dist (d_ring_rc, ring_len); indices wrap
 * modulo the claim grid extent like negative numba indices do. */
/* max_alive (all suppression calls): an upper bound of d_num_alive known to the caller, used only to size the
 * launch grid (0 = unknown: a grid for circle_cap).  d_skip (all three; may be NULL): int32[n_planes], planes with a
 * non-zero entry are left alone -- they were decided by mg_nms_sparse. */
int mg_nms_rounds(const int32_t* d_circles, int64_t circle_cap, const float* d_scores, const int32_t* d_alive,
                  const int32_t* d_num_alive, const int32_t* d_max_rc, int n_planes, int min_dist,
                  const int32_t* d_ring_rc, int ring_len, uint64_t* d_grid, int64_t grid_cap, uint8_t* d_state,
                  int32_t* d_undecided, int64_t undecided_stride, int n_rounds, int counters_clear,
                  const uint32_t* d_tie_keys, int64_t max_alive, const int32_t* d_skip, void* stream);

/* Before the rounds (optional, exact): of the alive circles that share a centre only the first in suppression
 * order (score desc, tie key asc) stays undecided, the others are marked rejected -- they have the same ring and
 * are rejected whatever happens to the first (utils.py:254-292).  One bid on the centre's own claim-grid cell,
 * which is restored before returning; d_state as for mg_nms_rounds. */
int mg_nms_same_centre(const int32_t* d_circles, int64_t circle_cap, const float* d_scores, const int32_t* d_alive,
                       const int32_t* d_num_alive, const int32_t* d_max_rc, int n_planes, int min_dist, uint64_t* d_grid,
                       int64_t grid_cap, uint8_t* d_state, const uint32_t* d_tie_keys, int64_t max_alive,
                       const int32_t* d_skip, void* stream);

/* After the rounds have converged: restore the all-ones claim grid under the rings of all alive
 * circles, so that the grid needs its full initialisation only once. */
int mg_nms_cleanup(const int32_t* d_circles, int64_t circle_cap, const float* d_scores, const int32_t* d_alive,
                   const int32_t* d_num_alive, const int32_t* d_max_rc, int n_planes, int min_dist,
                   const int32_t* d_ring_rc, int ring_len, uint64_t* d_grid, int64_t grid_cap, uint8_t* d_state,
                   int64_t max_alive, const int32_t* d_skip, void* stream);

/* The same greedy suppression (utils.py:254-292) decided from the circles alone, one workgroup per plane: circle i is
 * kept iff no circle j kept before it has a ring cell in common with it, i.e. iff c_i - c_j is in D = ring (-) ring for
 * no such j.  d_dbits: the bitmap of D, bit (dr + 2 d)(4 d + 1) + dc + 2 d set iff two rings of radius d = min_dist
 * whose centres differ by (dr, dc) share a cell (the caller builds it from the ring of mg_circle_points).  A plane's
 * alive circles are bucketed in LDS, a circle looks at the buckets around it; d_state gets 1 (kept) / 2 (dropped) for
 * every alive circle of a plane it decides and d_done[plane] = 1.  d_done[plane] = 0 -- the plane is left to
 * mg_nms_same_centre / mg_nms_rounds, untouched -- when it holds more than 12 288 alive circles, spans more than 9 216
 * buckets of 32 x 64, or a centre lies at row or col < -(min_dist + 1) (the reference's claim index would be negative
 * and wrap); every plane when min_dist > mg_nms_sparse_max_dist().  d_skip of the three calls above = this d_done:
 * they leave the planes alone that are decided (the cleanup only zeroes their circles' state bytes).  Needs no claim
 * grid and does not look at d_state before writing it.  A refused plane's state bytes are not written, alive circles'
 * included (so is a plane whose d_max_rc understates a centre); tests/test_gpu_nms_paths.py holds the kernel to these
 * limits, plane by plane. */
int mg_nms_sparse(const int32_t* d_circles, int64_t circle_cap, const float* d_scores, const int32_t* d_alive,
                  const int32_t* d_num_alive, const int32_t* d_max_rc, int n_planes, int min_dist, const uint32_t* d_dbits,
                  uint8_t* d_state, const uint32_t* d_tie_keys, int32_t* d_done, void* stream);
int mg_nms_sparse_max_dist(void);

/* Gather the kept circles in priority order (utils.py:195-199 output order):
 * d_out[n_planes][out_cap][3] int32 (row, col, r), d_out_scores, d_num_out[n_planes].
 * keep_all != 0 skips the state test (min_dist == 0: no suppression, utils.py:197).
 * Order: score descending, then d_tie_keys ascending, compared as UNSIGNED 32-bit (the unique keys reach bit 31 on large
 * images), or the index in d_circles when NULL.  At most out_cap rows per plane are written and d_num_out is clamped to
 * out_cap; which circles drop out then is unspecified.
 * d_scratch: int32[n_planes][3 * out_cap] work space (the kept circles' indices and 64-bit priority keys). */
#define MG_COLLECT_WALK 8192 /* workgroups per plane of the two gather kernels and of the suppression rounds (mg_nms_*) */
int mg_collect_circles(const int32_t* d_circles, int64_t circle_cap, const float* d_scores, const int32_t* d_alive,
                       const int32_t* d_num_alive, const uint8_t* d_state, int keep_all, int n_planes,
                       int32_t* d_out, float* d_out_scores, int64_t out_cap, int32_t* d_num_out,
                       int32_t* d_scratch, const uint32_t* d_tie_keys, int counters_clear, void* stream);

/* ------------------------------------------------------------------------------------
 * A12-A15, A18 labels, ROI gather, fg/bg masks, masked reductions
 * (utils.py:380-395, 60-80; find.py:561-602; README.md:21-22, identify.py:76-80)
 * ---------------------------------------------------------------------------------- */

/* circle_labels as a coverage count: d_labels[n_planes][h][w] int32 pre-set to -1;
 * beads d_beads[n_planes][bead_cap][3] (row, col, r), d_num_beads[n_planes];
 * d_halfwidths[(max_r+1)][2*max_r+1] from mg_disk_halfwidths (row r of the table). */
int mg_circle_labels(const int32_t* d_beads, int64_t bead_cap, const int32_t* d_num_beads, int n_planes, int h,
                     int w, const int32_t* d_halfwidths, int max_r, int32_t* d_labels, void* stream);

/* ROI gather + masks + reductions from a label map.  Every assay's image (C, T, h, w) of dtype (u8/u16/f32/f64: the
 * four are held to a NumPy restatement of the pass in tests/test_gpu_roi_edges.py, here and in mg_roi_segment_reduce);
 * beads (m, 3) with labels from time 0; window = bounding_box(col, row, L, w, h), 0 < L <= min(h, w), its L * L flag
 * bytes (+ 12 * L * ceil(L / 32) bytes of row masks in mg_roi_segment_reduce) within 60 000 bytes of LDS: L <= 244
 * here, <= 206 there -- MG_EINVAL beyond, nothing written.
 * Marker g belongs to assay d_marker_assay[g] (image base + assay * assay_stride
 * elements, labels base + assay * h * w) and owns label value d_marker_local[g].  Both index
 * arrays may be NULL (single assay, local index = g).  d_beads is (m, 3) for all markers.
 * Outputs: roi (m, C, T, L, L) same dtype; fg, bg (m, L, L) uint8 {0,1};
 * sums double[m][C][T][2] = {sum over fg, sum over bg} (exact for integer dtypes below 2^53),
 * counts int32[m][2] = {|fg|, |bg|}.  Any output pointer may be NULL. */
int mg_roi_gather_reduce_batched(const void* d_image, int dtype, int64_t assay_stride, int n_c, int n_t, int h, int w,
                                 const int32_t* d_beads, const int32_t* d_marker_assay,
                                 const int32_t* d_marker_local, int m, int roi_len, const int32_t* d_labels,
                                 void* d_roi, uint8_t* d_fg, uint8_t* d_bg, double* d_sums, int32_t* d_counts,
                                 void* stream);

/* d_offsets[0 .. n] = exclusive prefix sums of min(d_counts[i], cap) (int32, on the device): the d_assay_offsets of
 * mg_roi_segment_reduce from the per-assay bead counts mg_collect_circles left in device memory -- the ROI pass can
 * then be queued (with an upper bound for m) before the host has fetched the counts. */
int mg_counts_to_offsets(const int32_t* d_counts, int n, int cap, int32_t* d_offsets, void* stream);

/* The marker table a rank contributes to the final all-gather: row g of d_table[m][6 + 2 n_c] (float64)
 * = [assay_offset + assay, row, col, r, fg_count, bg_count, fg_sum[n_c], bg_sum[n_c]] of marker g, from the bead
 * tables (d_beads / bead_stride / d_assay_offsets as for mg_roi_segment_reduce: compact, or one padded row per assay)
 * and the counts (m, 2) / sums (m, n_c, n_t, 2) of the ROI pass at time index t_index.  m: the rows d_table holds; rows
 * beyond d_assay_offsets[n_assays] are left alone. */
#define MG_MARKER_TABLE_WALK 2048
int mg_marker_table(const int32_t* d_beads, int64_t bead_stride, const int32_t* d_assay_offsets, int n_assays, int m,
                    int assay_offset, const int32_t* d_counts, const double* d_sums, int n_c, int n_t, int t_index,
                    double* d_table, void* stream);

/* fg/bg segmentation + ROI gather + reductions WITHOUT a label map (find.py:561-602 with
 * utils.py:380-395 folded in): the masks come straight from the bead table.  A window pixel is
 * foreground iff it lies in the marker's own disk and in no other disk of its assay (labels == i),
 * background iff it lies in no disk (labels == -1).  d_beads (m, 3) = [row, col, r] of all markers,
 * assay-major; d_assay_offsets int32[n_assays + 1] delimits every assay's markers (marker g of assay
 * a has label value g - d_assay_offsets[a]).  One workgroup per marker, launched for m of them: m may be an upper
 * bound of d_assay_offsets[n_assays] (workgroups beyond it leave at once; markers beyond m are not worked on, the
 * outputs must hold m).  d_halfwidths / max_r as for mg_circle_labels (disks with
 * r < 2 or r > max_r cover nothing, as there).  bead_stride = 0: d_beads is that compact list;
 * bead_stride > 0: d_beads holds one padded row of bead_stride triples per assay (the layout
 * mg_collect_circles writes: the ROI pass can start from the device-resident tables while the host
 * is still fetching them); the outputs are compact either way.  time_major != 0: every assay's image
 * block is stored (n_t, n_c, h, w) instead of (n_c, n_t, h, w) -- a time-sharded single assay is gathered
 * where the flat-field pass left it, without a transposing copy; the outputs stay (channel, time)-ordered.
 * Outputs as mg_roi_gather_reduce_batched. */
int mg_roi_segment_reduce(const void* d_image, int dtype, int64_t assay_stride, int n_c, int n_t, int h, int w,
                          int time_major, const int32_t* d_beads, int64_t bead_stride, const int32_t* d_assay_offsets,
                          int n_assays, int m, const int32_t* d_order, int roi_len, const int32_t* d_halfwidths, int max_r,
                          void* d_roi, uint8_t* d_fg, uint8_t* d_bg, double* d_sums, int32_t* d_counts, void* stream);

/* mg_roi_segment_reduce for an image block in which only some channels have been corrected
 * (mg_flatfield_apply_stitch_planes): the channels c with bit c set in raw_channel_mask are gathered from the RAW
 * stack d_raw -- same layout and assay stride as d_image, un-tiled -- and flat-field corrected on the way, pixel for
 * pixel what the correction pass writes (one definition of the arithmetic, csrc/mg_flatcorr.h): scalar dark, flat
 * scalar (d_flat NULL) or a float32 (h, w) image, d_max2 / planes_per_group as for mg_flatfield_apply_stitch with
 * planes_per_group a multiple of n_c * n_t.  The other channels are read from d_image as they are.
 * Only the fast window kernel has this form: uint16 pixels, even roi_len <= 126, even w, 16-byte aligned d_image /
 * d_raw / d_flat, time_major == 0 (a time-major block is refused).  MG_EINVAL otherwise: the caller then corrects the
 * channels with the correction pass and calls mg_roi_segment_reduce. */
int mg_roi_segment_reduce_raw(const void* d_image, const void* d_raw, int dtype, int64_t assay_stride, int n_c, int n_t,
                              int h, int w, int time_major, int raw_channel_mask, double dark, double flat,
                              const float* d_flat, const double* d_max2, int planes_per_group,
                              const int32_t* d_beads, int64_t bead_stride, const int32_t* d_assay_offsets,
                              int n_assays, int m, const int32_t* d_order, int roi_len, const int32_t* d_halfwidths,
                              int max_r, void* d_roi, uint8_t* d_fg, uint8_t* d_bg, double* d_sums, int32_t* d_counts,
                              void* stream);

/* d_order[0 .. m) for mg_roi_segment_reduce (NULL there: markers are visited as listed): the markers of every assay
 * band by band (64 rows) and left to right inside a band, so that windows which share image lines are gathered at
 * about the same time and meet in the L2s (the reference walks its beads in score order, find.py:571-602; the order
 * of the work is free, every marker's outputs stay at the marker's index).  Tables as for mg_roi_segment_reduce. */
int mg_roi_window_order(const int32_t* d_beads, int64_t bead_stride, const int32_t* d_assay_offsets, int n_assays, int m,
                        int32_t* d_order, void* stream);

/* Masked median of an already gathered roi (m, C, T, L, L) of element type `dtype` (MG_U8 / U16 / F32 / F64):
 * roi.where(mask).median(dim=[roi_x, roi_y]) of identify.py:76-80 and filter.py:20-22, 74, 82 with numpy's nanmedian
 * semantics -- the mean of the two middle values (in float64), pixels outside the mask and NaN pixels ignored, NaN when
 * nothing is left.  The mask of marker g at timepoint t is the L x L bytes at d_mask + g * mask_stride_m +
 * t * mask_stride_t (elements; mask_stride_t = 0: one mask for all timepoints, as find_beads replicates its geometry,
 * find.py:585-586; chips searched at several timesteps have a mask per timepoint, find.py:119-140).
 * d_median double[m][C][T].  Exact: radix select on the order-preserving bit pattern of the values.
 * Served by the kernel of mg_roi_masked_stats (below) in its median mode: one read of a window whose keys fit the LDS
 * budget, the two middle ranks selected directly (one where the count is odd), one double written per window.  Its
 * limits are that entry point's -- MG_EINVAL, with nothing written: a null pointer, an unknown dtype, m < 0,
 * n_c / n_t / roi_len <= 0, roi_len > MG_ROISTATS_MAX_LEN, m * n_c * n_t >= 2^31, a negative stride (n_c * n_t itself
 * is no longer limited to 65535).  m = 0 returns MG_OK and writes nothing.  One kernel launch. */
int mg_roi_masked_median(const void* d_roi, int dtype, const uint8_t* d_mask, int64_t mask_stride_m,
                         int64_t mask_stride_t, int m, int n_c, int n_t, int roi_len, double* d_median, void* stream);

/* Every statistic that roi.where(mask).<reduction>(dim=[roi_x, roi_y]) can ask for, from one read of each window
 * (README.md:21-22; the robust intensities of a masked ROI: an upper percentile of the foreground, the spread of the
 * background, a saturation check by max).  d_roi (m, C, T, L, L) and the masks as for mg_roi_masked_median.  A pixel
 * takes part iff its mask byte is non-zero and its value is not NaN; n = the number of such pixels of one (g, c, t).
 * q: HOST array of n_q fractions in [0, 1], 0 <= n_q <= MG_ROISTATS_MAX_Q, read during the call.
 *   d_count int32[m][C][T]            n
 *   d_stats double[m][C][T][4]        {sum, m2, min, max}: m2 = sum (x - mean)^2 with mean = sum / n, every operation
 *                                     in float64 and none contracted (where all n values are equal the mean is
 *                                     that value: m2 = 0 exactly); {0, 0, NaN, NaN} for n = 0.  For integer pixels
 *                                     sum is exact; for float pixels sum and m2 are accumulated in an order fixed by
 *                                     the launch shape (no floating-point atomics): every call gives the same bits.
 *   d_order double[m][C][T][n_q][2]   {sorted[lo], sorted[hi]} of the n values: pos = (double)(n - 1) * q,
 *                                     lo = floor(pos), hi = min(lo + 1, n - 1); NaN for n = 0.  Exact: radix select on
 *                                     the order-preserving bit pattern.  May be NULL when n_q = 0.
 * One workgroup per window.  A window whose keys (4 bytes a pixel, 8 for MG_F64) fit MG_ROISTATS_LDS_KEY_BYTES of LDS is
 * read from global memory once and everything after the first pass runs out of LDS; a larger one is read again for m2
 * and for every selection (mg_roi_masked_stats_keys_in_lds tells which; the results are the same).
 * MG_EINVAL, with nothing written: a null pointer where one is needed, an unknown dtype, m < 0, n_c / n_t / roi_len <= 0,
 * roi_len > MG_ROISTATS_MAX_LEN (pixel indices are int), m * n_c * n_t >= 2^31, a negative stride, n_q outside
 * [0, MG_ROISTATS_MAX_Q], a q that is NaN or outside [0, 1].  m = 0 returns MG_OK and writes nothing.  One kernel
 * launch; no allocation, no synchronisation. */
#define MG_ROISTATS_MAX_Q 16
#define MG_ROISTATS_LDS_KEY_BYTES 49152
#define MG_ROISTATS_MAX_LEN 32768
int mg_roi_masked_stats(const void* d_roi, int dtype, const uint8_t* d_mask, int64_t mask_stride_m,
                        int64_t mask_stride_t, int m, int n_c, int n_t, int roi_len, const double* q, int n_q,
                        int32_t* d_count, double* d_stats, double* d_order, void* stream);
/* 1 if a window of roi_len x roi_len pixels of `dtype` keeps its keys in LDS, 0 if it takes the path that selects from
 * global memory; MG_EINVAL for an unknown dtype or a roi_len that mg_roi_masked_stats refuses.  Host only. */
int mg_roi_masked_stats_keys_in_lds(int dtype, int roi_len);

/* Radial intensity profiles of an already gathered roi (profile_rois).  NOT in the reference: its reductions stop at one
 * number per mask, and the markers are round -- ring against core of a bead, disk or doughnut of a button, the radius at
 * which a bead falls to the background.  tests/radial_ref.py restates the contract in plain Python.
 * d_roi (m, C, T, L, L) of `dtype`, the mask as for mg_roi_masked_stats (d_mask may be NULL: every pixel).  d_centre:
 * {cy, cx} of window (g, t) in window coordinates, int32 at d_centre + g * centre_stride_m + t * centre_stride_t
 * (elements; a time stride of 0: one centre for all timepoints).  Centres and edges are integers in units of
 * 1 / MG_PROFILE_SUBPIXEL pixel; edges: HOST array of n_rings + 1, read during the call.  With S = MG_PROFILE_SUBPIXEL,
 * all in exact integer arithmetic:
 *   d2(i, j) = (i S - cy)^2 + (j S - cx)^2; pixel (i, j) belongs to ring k iff edges[k]^2 <= d2 < edges[k + 1]^2 (a
 *   pixel on an edge goes to the outer ring; inside edges[0] or from edges[n_rings] on it belongs to none); it takes
 *   part iff its mask byte is non-zero (or d_mask is NULL) and its value is not NaN.
 * Limits, so that 32 unsigned bits hold d2: roi_len <= MG_PROFILE_MAX_LEN, 0 <= edges[0] < edges[1] < ... <= MG_PROFILE_MAX_EDGE,
 * and MG_PROFILE_CENTRE_MIN = -1024 S <= cy, cx <= 2048 S = MG_PROFILE_CENTRE_MAX -- centres are device data and cannot be refused: the kernel clamps them into that range.
 *   d_count   int32[m][C][T][n_rings]       the pixels that take part
 *   d_moments double[m][C][T][n_rings][2]   {sum x, sum x^2}; an empty ring: {0, 0}, count 0
 * Integer pixels: both moments are accumulated exactly in 64-bit integers (integer LDS atomics) and converted once: the
 * correctly rounded exact values.  Float pixels: float64, nothing contracted, no floating-point atomic anywhere -- runs
 * of one ring along a row are folded by a segmented scan over the lanes and added to per-wave slots in an order fixed
 * by the launch shape: every call gives the same bits.  One workgroup per (marker, time); the ring of a pixel is found
 * once and kept as a byte in LDS for the other channels where L <= 128.
 * MG_EINVAL, with nothing written: a null pointer where one is needed, an unknown dtype, m < 0, n_c / n_t / roi_len <= 0,
 * roi_len > MG_PROFILE_MAX_LEN, n_rings outside [1, MG_PROFILE_MAX_RINGS], edges not strictly increasing or out of
 * range, m * n_c * n_t >= 2^31, a negative stride.  m = 0 returns MG_OK and writes nothing.  One kernel launch; no
 * allocation, no synchronisation. */
#define MG_PROFILE_MAX_RINGS 128
#define MG_PROFILE_SUBPIXEL 16
#define MG_PROFILE_MAX_LEN 1024
#define MG_PROFILE_CENTRE_MIN (-16384) /* -1024 S */
#define MG_PROFILE_CENTRE_MAX 32768    /* 2048 S */
#define MG_PROFILE_MAX_EDGE 46340      /* the largest integer whose square 31 bits hold */
int mg_roi_radial_profile(const void* d_roi, int dtype, const uint8_t* d_mask, int64_t mask_stride_m,
                          int64_t mask_stride_t, const int32_t* d_centre, int64_t centre_stride_m,
                          int64_t centre_stride_t, const int32_t* edges, int n_rings, int m, int n_c, int n_t,
                          int roi_len, int32_t* d_count, double* d_moments, void* stream);

/* Per-pixel linear unmixing of an already gathered roi, reduced per bead (identify_mrbles(unmix="pixel")).  NOT in the
 * reference, which unmixes one number per bead and channel (identify.py:72-83); this is the published MRBLEs analysis:
 * unmix every pixel, form the ratio image, take the median of the ratio inside the bead and keep its spread.
 * tests/unmix_ref.py restates the contract in plain NumPy.
 * d_roi (m, C, T, L, L) of `dtype`, the mask as for mg_roi_masked_stats (d_mask may be NULL: every pixel).
 * channels: HOST array of n_k different indices into C, 1 <= n_k <= MG_UNMIX_MAX_CHANNELS; matrix: HOST array
 * double[n_ln][n_k], 1 <= n_ln <= MG_UNMIX_MAX_LN, every entry finite; q: HOST array of n_q fractions in [0, 1],
 * 0 <= n_q <= MG_UNMIX_MAX_Q; all three are read during the call.  d_offset: device double[m][C][T], indexed by the
 * ORIGINAL channel (the output of mg_roi_masked_median as it is), or NULL: zeros.
 * For pixel p of window (g, t), everything in float64 and nothing contracted:
 *   x_j = (double)roi[g, channels[j], t, p] - offset[g, channels[j], t]                       j = 0 .. n_k - 1
 *   v_k = (...((matrix[k][0] * x_0) + matrix[k][1] * x_1) + ...) + matrix[k][n_k-1] * x_{n_k-1}   k = 0 .. n_ln - 1
 *   r_k = v_k / v_0                                                                           k = 1 .. n_ln - 1
 * every product rounded, then every sum, left to right in the order of `channels`; the division is IEEE.  The derived
 * values of a pixel, in this order: v_0 .. v_{n_ln-1}, r_1 .. r_{n_ln-1}; D = 2 n_ln - 1 of them.  A derived value
 * takes part iff the pixel's mask byte is non-zero (or d_mask is NULL) and the value is not NaN: 0 / 0 drops out,
 * x / 0 = +-inf stays, as infinities stay in mg_roi_masked_stats.
 *   d_count int32[m][T][D]            n, the values that take part
 *   d_sum   double[m][T][D]           their sum in float64, accumulated in an order fixed by the launch shape (no
 *                                     floating-point atomics): every call gives the same bits; 0 where n = 0
 *   d_order double[m][T][D][n_q][2]   {sorted[lo], sorted[hi]}: pos = (double)(n - 1) * q, lo = floor(pos),
 *                                     hi = min(lo + 1, n - 1); NaN for n = 0.  Exact: radix select on the
 *                                     order-preserving bit pattern (-0.0 sorts below +0.0), the contract of
 *                                     mg_roi_masked_stats.  May be NULL when n_q = 0.
 * One workgroup per (marker, time); the mask is read once.  The n_ln volumes of the masked pixels are kept in LDS, 8
 * bytes each, where n_masked * n_ln * 8 <= MG_UNMIX_LDS_KEY_BYTES (two workgroups of that size fit a compute unit's
 * 160 KiB), and the ratios are formed from them during the selection passes; a window with more masked pixels computes
 * its values again from global memory in each pass (mg_roi_unmix_keys_in_lds tells which; the results are the same bits).
 * MG_EINVAL, with nothing written: a null pointer where one is needed, an unknown dtype, m < 0, C / T / roi_len <= 0,
 * roi_len > MG_UNMIX_MAX_LEN, n_k / n_ln / n_q out of range, a channel outside [0, C) or repeated, a matrix entry that
 * is not finite, a q that is NaN or outside [0, 1], m * T * D >= 2^31 (or m * C * T), a negative stride.  m = 0 returns
 * MG_OK and writes nothing.  One kernel launch; no allocation, no synchronisation. */
#define MG_UNMIX_MAX_CHANNELS 16
#define MG_UNMIX_MAX_LN 8
#define MG_UNMIX_MAX_Q 8
#define MG_UNMIX_MAX_LEN 1024
#define MG_UNMIX_LDS_KEY_BYTES 79872
int mg_roi_unmix_stats(const void* d_roi, int dtype, const uint8_t* d_mask, int64_t mask_stride_m, int64_t mask_stride_t,
                       int m, int n_c, int n_t, int roi_len, const int* channels, int n_k, const double* matrix, int n_ln,
                       const double* d_offset, const double* q, int n_q, int32_t* d_count, double* d_sum, double* d_order,
                       void* stream);
/* 1 if a window with n_masked pixels under its mask keeps its n_ln volumes in LDS, 0 if it takes the path that computes
 * them again from global memory; MG_EINVAL for an n_ln that mg_roi_unmix_stats refuses or n_masked < 0.  Host only. */
int mg_roi_unmix_keys_in_lds(int n_ln, int64_t n_masked);

/* The same arithmetic over whole planes: lanthanide images of a chip or a bead field.  d_src: plane (c, t) of `dtype`,
 * (h, w) contiguous, at d_src + c * chan_stride + t * time_stride elements; channels and matrix as above; offset: HOST
 * double[n_k], one finite constant per USED channel, or NULL: zeros.  d_dst float32 (n_out, n_t, h, w), contiguous:
 * ratios = 0: n_out = n_ln, the planes (float)v_k; ratios = 1: n_out = 2 n_ln - 1, those followed by (float)r_k,
 * k = 1 .. n_ln - 1.  Computed in float64 exactly as above and cast once; a NaN pixel gives NaN.  A streaming kernel:
 * every source pixel of a used channel is read once, every output written once, four pixels per load and store where
 * the planes' addresses allow, pixel by pixel otherwise and for the last h w % 4.
 * MG_EINVAL, with nothing written: a null pointer where one is needed, a pointer not aligned to its element, an unknown
 * dtype, n_c / n_t / h / w <= 0 (h above 2^30, w above 2^20), n_k / n_ln out of range, a channel outside [0, n_c) or
 * repeated, a matrix entry or an offset that is not finite, ratios other than 0 / 1, n_out * n_t >= 2^31, a negative
 * stride.  One kernel launch; no allocation, no synchronisation. */
#define MG_UNMIX_PLANES_WALK_PER_PLANE 8192 /* workgroups of 256 lanes x 4 pixels along one time plane */
int mg_unmix_planes(const void* d_src, int dtype, int64_t chan_stride, int64_t time_stride, int n_c, int n_t, int h, int w,
                    const int* channels, int n_k, const double* matrix, int n_ln, const double* offset, int ratios,
                    float* d_dst, void* stream);

/* Data-driven fg / bg masks of an already gathered roi (segment_rois).  NOT in the reference, whose masks are drawn
 * shapes -- the fitted circle (find.py:561-586), disk and annulus (find.py:383-400); this is the threshold / dilation /
 * erosion family that BASELINE.json's north star names for the fg/bg masks.  tests/segment_ref.py restates the contract
 * in NumPy + scipy.ndimage and the kernel equals it bit for bit.
 * d_roi points at the first window of ONE channel, element type `dtype`; window (g, t), roi_len x roi_len contiguous
 * pixels, is at d_roi + g * stride_m + t * stride_t (elements).  The drawn masks fg0 / bg0 and the optional `allowed`
 * (d_allowed may be NULL) are roi_len x roi_len bytes at their pointer + g * stride_m + t * stride_t of their own (a
 * time stride of 0: one mask for all timepoints); a byte is set iff it is non-zero.  S = the 3x3 all-ones structuring
 * element, outside the window is off.  Per window:
 *   1. lo, hi = min, max of the non-NaN pixels as float64.  The window is UNSEGMENTED where hi - lo is not finite or
 *      not > 0, or there is no such pixel.
 *   2. b(v) = floor((255.0 * (v - lo)) / (hi - lo)) in float64, one operation at a time (to_uint8's order, utils.py:24-26),
 *      at most 255.  A NaN pixel has no bin and is off.
 *   3. use_otsu: h = the histogram of b, N = sum h, Stot = sum i h[i]; for k = 0 .. 254 with w0 = sum_{i<=k} h > 0 and
 *      w1 = N - w0 > 0: d = Stot w0 - N sum_{i<=k} i h[i] (exact, int64), value = (d * d) / (double)(w0 w1); k* = the
 *      smallest k of the largest value; on = b > k*; reported threshold lo + ((k* + 1) * (hi - lo)) / 255.0.
 *      Otherwise on = v > threshold and that number is reported.
 *   4. opened = open_radius erosions of `on` by S, then open_radius dilations; opened &= allowed where given.
 *   5. fg = opened & fg0, then max_grow times fg = dilate(fg, S) & opened.
 *   6. Where the window is unsegmented or sum(fg) < max(min_area, 1): fg0 and bg0 are written out (as 0 / 1),
 *      segmented = 0, threshold = NaN if unsegmented and the threshold found otherwise.
 *   7. Else bg = bg0 & ~(bg_guard dilations of on | fg), segmented = 1.
 * d_fg, d_bg uint8 [m][n_t][roi_len][roi_len] (0 / 1, every byte written once), d_threshold double[m][n_t], d_counts
 * int32[m][n_t][2] = {sum fg, sum bg} of what was written, d_segmented uint8[m][n_t].
 * One workgroup per window: bins as bytes and every mask as a bit plane in LDS (at most 40 KB), integer histogram and
 * prefix sums, a total order in the arg-max -- the same bits on every call.  MG_EINVAL, with nothing launched: a null
 * pointer where one is needed, an unknown dtype, m < 0, n_t <= 0, roi_len outside 1 .. MG_SEGMENT_MAX_LEN,
 * m * n_t >= 2^31, a negative stride, open_radius / max_grow / bg_guard outside 0 .. MG_SEGMENT_MAX_OPEN / _GROW /
 * _GUARD, min_area < 0, a NaN threshold with use_otsu = 0.  m = 0 returns MG_OK and writes nothing.  One kernel launch;
 * no scratch buffer, no allocation, no synchronisation. */
#define MG_SEGMENT_MAX_LEN 128
#define MG_SEGMENT_MAX_OPEN 8
#define MG_SEGMENT_MAX_GROW 32
#define MG_SEGMENT_MAX_GUARD 16
int mg_roi_threshold_masks(const void* d_roi, int dtype, int64_t stride_m, int64_t stride_t,
                           const uint8_t* d_fg0, int64_t fg_stride_m, int64_t fg_stride_t,
                           const uint8_t* d_bg0, int64_t bg_stride_m, int64_t bg_stride_t,
                           const uint8_t* d_allowed, int64_t al_stride_m, int64_t al_stride_t,
                           int m, int n_t, int roi_len, int use_otsu, double threshold,
                           int open_radius, int max_grow, int bg_guard, int min_area,
                           uint8_t* d_fg, uint8_t* d_bg, double* d_threshold, int32_t* d_counts, uint8_t* d_segmented,
                           void* stream);

/* Sub-pixel circle fit of every marker of an already gathered roi (refine_markers, refine="edge").  NOT in the
 * reference, whose finders stop at the integer circle of the RANSAC vote and drop its radius (find.py:561-586,
 * find.py:383-400).  A radial edge search along n_rays rays about the found circle, then an algebraic (Kasa) circle fit
 * with one rejection round.  tests/refine_ref.py restates the contract in plain NumPy loops and the kernel equals it
 * bit for bit.
 * d_roi points at the first window of ONE channel, element type `dtype`; window (g, t), roi_len x roi_len contiguous
 * pixels, is at d_roi + g * roi_stride_m + t * roi_stride_t (elements).  d_circle: the start circle {cy, cx, r} of window
 * (g, t) in window coordinates, int32 in units of 1 / MG_PROFILE_SUBPIXEL pixel, at d_circle + g * circle_stride_m +
 * t * circle_stride_t (elements; a time stride of 0: one circle for all timepoints).  Circles are device data and cannot
 * be refused: cy, cx are clamped to mg_roi_radial_profile's range [-1024, 2048] pixels and r to [0, 1024] pixels.
 * d_cs: DEVICE double[n_rays][2] = {cos, sin}(2 pi k / n_rays), computed by the host; the kernel calls no trigonometric
 * function and takes no square root.  With K = n_rays, L = roi_len, cy, cx, r now in pixels (the integers / 16.0), all in
 * float64, every operation rounded once, left to right as written, nothing contracted:
 *   1. J = 4 reach + 1 samples per ray at rho_j = (r - reach) + 0.5 j; j_lo = the first j with rho_j >= 0, the same for
 *      all rays of the window.  Sample (k, j) lies at y = cy + rho_j * sin_k, x = cx + rho_j * cos_k.
 *   2. iy = floor(y), ix = floor(x), fy = y - iy, fx = x - ix.  The sample is inside iff 0 <= iy, iy + 1 <= L - 1 and the
 *      same in x (a NaN position is outside).  Its value, from the pixels W converted to float64:
 *      (W[iy][ix] * (1 - fx) + W[iy][ix+1] * fx) * (1 - fy) + (W[iy+1][ix] * (1 - fx) + W[iy+1][ix+1] * fx) * fy.
 *      A ray is USABLE iff every sample j >= j_lo is inside and its value is finite.
 *   3. d_j = v_{j+1} - v_{j-1} for j_lo + 1 <= j <= J - 2 (at least one j).
 *   4. polarity 0 (auto): P+ = sum_k max_j d_j and P- = sum_k max_j (-d_j), both over the usable rays in ascending k;
 *      the polarity is +1 (brighter outside) iff P+ >= P-, else -1.  polarity +1 / -1: as given.  e_j = polarity * d_j.
 *   5. j* = the first arg-max of e_j.  The ray is VALID iff it is usable, e_{j*} > 0 and j* is neither the first nor the
 *      last derivative index.  With e-, e0, e+ = e_{j*-1}, e_{j*}, e_{j*+1}: delta = (0.5 * (e- - e+)) / ((e- - 2 e0) + e+),
 *      rho_k = rho_{j*} + 0.5 * delta, strength w_k = e0.
 *   6. KEPT: the valid rays with w_k >= min_strength * max_k w_k.  Fewer than min_rays: status 1.
 *   7. Fit over a set of n rays, every sum in ascending k: u = rho_k * cos_k, v = rho_k * sin_k (offsets from the start
 *      centre); ub = (sum u) / n, vb = (sum v) / n; u' = u - ub, v' = v - vb, z = u' u' + v' v'; Suu = sum u' u',
 *      Suv = sum u' v', Svv = sum v' v', Suz = sum u' z, Svz = sum v' z; det = Suu Svv - Suv Suv;
 *      a' = (0.5 * (Suz Svv - Svz Suv)) / det, b' = (0.5 * (Svz Suu - Suz Suv)) / det; a = ub + a', b = vb + b';
 *      R2 = (a' a' + b' b') + (Suu + Svv) / n.  The fit FAILS where det > 0 or R2 > 0 does not hold.
 *   8. Fit the kept set.  g_k = ((u - a)^2 + (v - b)^2) - R2; ray k is dropped iff g_k g_k > (4 (reject reject)) R2 -- the
 *      geometric residual against `reject` pixels, without a square root.  If a ray was dropped and at least min_rays
 *      remain, the rest is fitted again and is the final set; otherwise the kept set is, with its fit.  With g_k of the
 *      final fit: msq = (sum g_k g_k) / ((4 R2) n), mean strength = (sum w_k) / n.
 *   9. status: 0 ok; 1 too few rays (rule 6); 2 degenerate -- a fit failed, or a, b, R2, msq or the mean strength is not
 *      finite; 3 out of reach -- a a + b b > reach^2, or R2 outside [max(r - reach, 0)^2, (r + reach)^2].  Tested in
 *      this order.
 *   d_info int32[m][n_t][4]    {status, n_used, n_valid, polarity}: the size of the final set (of the kept set for
 *                              status 1), the number of valid rays, the polarity used
 *   d_fit  double[m][n_t][5]   {b (dy), a (dx), R2, msq, mean strength}; all five the quiet NaN 0x7FF8000000000000
 *                              where status != 0
 * One workgroup of 256 lanes per (marker, time): the samples as float64 in LDS (at most 33 KB), one lane per ray for
 * rules 3 and 5 and for the terms of rules 7 and 8, one lane per ordered sum -- the same bits on every call.  The launch is not capped: one workgroup
 * per window, as mg_roi_radial_profile and mg_roi_threshold_masks launch theirs.
 * MG_EINVAL, with nothing written: a null pointer, an unknown dtype, m < 0, n_t <= 0, roi_len outside
 * 1 .. MG_REFINE_MAX_LEN, m * n_t >= 2^31, a negative stride, n_rays outside [8, MG_REFINE_MAX_RAYS], reach outside
 * [1, MG_REFINE_MAX_REACH], polarity outside {-1, 0, 1}, reject not finite or not > 0, min_strength outside [0, 1],
 * min_rays outside [3, n_rays].  m = 0 returns MG_OK and writes nothing.  One kernel launch; no allocation, no
 * synchronisation. */
#define MG_REFINE_MAX_RAYS 128
#define MG_REFINE_MAX_REACH 8
#define MG_REFINE_MAX_LEN 1024
#define MG_REFINE_MAX_RADIUS 16384 /* 1024 S */
int mg_roi_refine_circles(const void* d_roi, int dtype, int64_t roi_stride_m, int64_t roi_stride_t,
                          const int32_t* d_circle, int64_t circle_stride_m, int64_t circle_stride_t,
                          const double* d_cs, int n_rays, int m, int n_t, int roi_len, int reach, int polarity,
                          double reject, double min_strength, int min_rays, int32_t* d_info, double* d_fit,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * A16 / A17 ButtonFinder helpers (find.py:205-402, 632-677)
 * ---------------------------------------------------------------------------------- */

/* cluster_1d (find.py:632-677): the cost of every integer offset in [0, n_offsets) for
 * n_clusters equal-width clusters over the ascending d_sorted_points (float64):
 * sum_k var_k * sqrt(ideal_k) + penalty * (ideal_k - n_k)^2, empty clusters take the largest
 * var.  The caller takes the first minimum (strict <, find.py:666).  d_costs double[n_offsets]. */
int mg_cluster1d_costs(const double* d_sorted_points, int n_points, int n_offsets, int n_clusters,
                       double cluster_length, const double* d_ideal, double penalty, double* d_costs, void* stream);

/* fg / bg masks of find_rois (find.py:383-400): fg[g] = cv.circle(filled, radius d_radii[g]),
 * bg[g] = annulus(outer_r, inner_r), centred at d_centers[g] = (row, col) inside the
 * roi_len x roi_len window.  d_cv_halfwidths[(max_table_r + 1)][hw_stride]: row r holds
 * mg_cv_disk_halfwidths(r).  Outputs uint8 [m][roi_len][roi_len]. */
int mg_button_masks(const int32_t* d_centers, const int32_t* d_radii, int m, int roi_len, int outer_r, int inner_r,
                    const int32_t* d_cv_halfwidths, int hw_stride, int max_table_r, uint8_t* d_fg, uint8_t* d_bg,
                    void* stream);

/* Masked sums with explicit masks: roi (m, n_c, n_t, L, L); fg / bg uint8, the L x L bytes of marker g at timepoint t
 * at d_xx + g * xx_stride_m + t * xx_stride_t (strides >= 0 in bytes; a time stride of 0: one mask for all timepoints),
 * as mg_roi_masked_stats reads its mask -> d_sums double[m][n_c][n_t][2] = {fg sum, bg sum}; d_counts (optional)
 * int32[m][n_tm][2] = {fg count, bg count} of timepoints 0 .. n_tm - 1, n_tm = 1 or n_t.  n_c * n_t <= 65535. */
int mg_masked_sums(const void* d_roi, int dtype, const uint8_t* d_fg, int64_t fg_stride_m, int64_t fg_stride_t,
                   const uint8_t* d_bg, int64_t bg_stride_m, int64_t bg_stride_t, int m, int n_c, int n_t, int roi_len,
                   double* d_sums, int32_t* d_counts, int n_tm, void* stream);

/* ------------------------------------------------------------------------------------
 * Measurement aid ("confirm with a measured streaming-copy ceiling on the box")
 * ---------------------------------------------------------------------------------- */

/* One streaming pass over n_bytes (a multiple of 16, 16-byte aligned buffers) by this library's own 16-byte-per-lane
 * grid-stride kernel on `blocks` workgroups of 256 (1 .. 65535; 0: one 16-byte access per lane, n_bytes / 4096
 * workgroups): mode 0 copies d_src to d_dst, mode 1 only reads d_src (d_sink: one word, written only if a lane's
 * words XOR to one particular value -- it keeps the loads alive), mode 2 only writes d_dst.  The caller times it
 * (HIP events). */
int mg_stream_probe(const void* d_src, void* d_dst, int64_t n_bytes, int mode, uint32_t* d_sink, int blocks, void* stream);

/* ------------------------------------------------------------------------------------
 * Host side of the streamed ingest (reader.py:265-292: the reference maps every TIFF
 * page to its own dask block and tifffile reads it when the block is computed)
 * ---------------------------------------------------------------------------------- */

/* Positional reads of n byte runs -- run i = nbytes[i] bytes at offsets[i] of the open file fds[i], into dsts[i]
 * (HOST pointers; page-locked blocks in the product, so the upload that follows is asynchronous) -- by n_threads
 * threads (1 .. 64) that take runs by ticket.  No GPU work, no stream; the call returns when every run is in place.
 * Returns MG_OK; MG_EINVAL for a bad argument; MG_EIO when a read failed or met the end of its file: failed[0] = the
 * run's index, failed[1] = errno (0: end of file).  `failed` may be NULL. */
int mg_host_read_runs(const int32_t* fds, const int64_t* offsets, const int64_t* nbytes, void* const* dsts, int n,
                      int n_threads, int64_t* failed);
/* The mirror image for the results of a streamed run (accessor.py:18-35: the reference spills every assay's roi / fg / bg
 * to a zarr store; here mg.save's NetCDF writer puts a variable's bytes -- already big-endian, swapped on the device --
 * where the header says): run i = nbytes[i] bytes from srcs[i] (HOST pointers) to offsets[i] of the open file fds[i].
 * Same threads, return values and `failed` as mg_host_read_runs. */
int mg_host_write_runs(const int32_t* fds, const int64_t* offsets, const int64_t* nbytes, void* const* srcs, int n,
                       int n_threads, int64_t* failed);

/* ------------------------------------------------------------------------------------
 * plot.overview (plot/image.py:52-168: the pixel work of imshow -- pyramid, one additive colour per channel, the
 * label map of the foreground masks -- as an RGB picture made on the device; tests/plot_ref.py restates both entries)
 * Below s = 2^level, hk = ceil(h / s), wk = ceil(w / s).
 * ---------------------------------------------------------------------------------- */
#define MG_OVERVIEW_MAX_LEVEL 6
#define MG_OVERVIEW_MAX_CHANNELS 16
#define MG_OVERVIEW_WALK 2048      /* mg_render_overview: workgroups of 256 items (a run of output pixels of one row) */
#define MG_IMAGE_LABELS_WALK 8192  /* mg_roi_image_labels: workgroups of 256 items (four mask pixels of one window row) */

/* Label map of the foreground masks in image coordinates (roi_to_image_labels, plot/image.py:157-168).  The mask of
 * marker g at timepoint t is the roi_len x roi_len bytes at d_fg + g * mask_stride_m + t * mask_stride_t (elements;
 * mask_stride_t = 0: one mask for all timepoints), its window's origin d_origin[g][t] = (top, left), int32 (m, n_t, 2).
 * d_labels int32 (n_t, hk, wk), zeroed by the caller: every set mask pixel (ry, rx) claims
 * labels[t, (top + ry) >> level, (left + rx) >> level] with g + 1 and the largest claim wins (atomicMax: the same bits
 * on every call); at level 0 that is the reference's overwrite with g ascending.  Claims outside the image are
 * dropped.  m = 0 is legal and launches nothing.  MG_EINVAL, with nothing launched: m < 0, n_t / roi_len / h / w < 1,
 * level outside 0 .. MG_OVERVIEW_MAX_LEVEL, a negative stride, a null pointer.  One kernel launch. */
int mg_roi_image_labels(const uint8_t* d_fg, int64_t mask_stride_m, int64_t mask_stride_t, const int32_t* d_origin, int m,
                        int n_t, int roi_len, int level, int h, int w, int32_t* d_labels, void* stream);

/* The composite.  d_image: plane (c, t) of `dtype`, (h, w) contiguous, at d_image + c * chan_stride + t * time_stride
 * elements.  limits double[n_c][2] = (lo, hi), colors double[n_c][3] in [0, 1]: HOST pointers, read during the call.
 * d_out uint8 (n_t, hk, wk, 3).  Per output pixel, in float64, one operation at a time: per channel the sum of the
 * in-image pixels of its s x s block (exact for MG_U8 / MG_U16; float pixels row by row from the top, each row from the
 * left), mean = sum / n, u = (mean - lo) / (hi - lo), u = 0 where hi <= lo, u is NaN or u < 0, u = 1 where u > 1,
 * acc[j] = min(acc[j] + u * colors[c][j], 1) with the channels ascending; then the overlay from d_labels (the map of
 * the same level; NULL with overlay 0) and d_table uint8 (n_marks, n_t, 3), the colour of marker g at timepoint t:
 * overlay 2 ("fill"): where 0 < lab <= n_marks, acc = (1 - alpha) * acc + alpha * table[lab - 1, t] / 255; overlay 1
 * ("outline"): the same with alpha = 1, only where one of the four neighbours in the label map holds another label
 * (0 outside the picture); overlay 0: none.  byte = floor(255 * acc + 0.5).  MG_EINVAL, with nothing launched: a null
 * image / output / limits / colors, an unknown dtype, n_c outside 1 .. MG_OVERVIEW_MAX_CHANNELS, n_t / h / w < 1, level
 * outside 0 .. MG_OVERVIEW_MAX_LEVEL, a negative stride, an unknown overlay, alpha or a colour outside [0, 1], an
 * overlay without labels, table or markers.  One kernel launch; no allocation, no synchronisation. */
int mg_render_overview(const void* d_image, int dtype, int64_t chan_stride, int64_t time_stride, int n_c, int n_t, int h,
                       int w, int level, const double* limits, const double* colors, const int32_t* d_labels,
                       const uint8_t* d_table, int n_marks, int overlay, double alpha, uint8_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------
 * plot.roishow and plot.percentile_limits (plot/image.py:14-49: the montage of every marker's window, bg in red and fg
 * in green on top; exact percentiles of a resident stack as contrast limits; tests/roishow_ref.py restates both)
 * ---------------------------------------------------------------------------------- */
#define MG_PERCENTILE_MAX_PREFIXES 4
#define MG_PERCENTILE_MAX_BITS 11
#define MG_PERCENTILE_WALK 2048 /* mg_percentile_histogram: workgroups; each walks its share of the chunks */
#define MG_MONTAGE_WALK 65536   /* mg_render_roi_montage: workgroups of 256 output pixels */

/* One read-once histogram pass of the radix selection of order statistics (hotpath.percentiles picks the bins between
 * passes).  Data: n0 * n1 units of unit_len contiguous elements of `dtype`, unit (i0, i1) at d_data + i0 * stride0 +
 * i1 * stride1 (elements; 0 is legal: a broadcast view).  The key of a value: the value for u8 (8 bits) and u16 (16
 * bits); for f32, and f64 rounded to f32, the 32 bits with the sign bit flipped (positive) or all bits flipped
 * (negative), -0 as +0; NaN has no key and is never counted.  n_prefixes = 0, the first pass: shift + bits = key bits,
 * every key is counted at d_hist[key >> shift].  n_prefixes in 1 .. MG_PERCENTILE_MAX_PREFIXES, a refinement:
 * prefix_shift = shift + bits, the prefixes (a host array, distinct, each below 2^(key bits - prefix_shift)) name the
 * leading bits selected so far; a key with key >> prefix_shift == prefixes[q] is counted at d_hist[q * 2^bits + ((key
 * >> shift) & (2^bits - 1))], every other key nowhere.  d_hist: uint64 counters, max(n_prefixes, 1) * 2^bits of
 * them, zeroed by the caller; the pass adds to them (LDS tables per workgroup, equal keys of a wave gathered before the
 * atomic, one uint64 atomic per non-empty bin and workgroup).  n0, n1 or unit_len = 0 is legal and launches nothing.
 * MG_EINVAL, with nothing launched: an unknown dtype, a null pointer, a negative count or stride, bits outside 1 ..
 * MG_PERCENTILE_MAX_BITS, shift < 0, shift + bits beyond the key, a first pass that leaves leading bits out, a
 * prefix_shift other than shift + bits, a prefix out of range or named twice, a stack so large that one workgroup's
 * share of it could pass the 2^32 of its uint32 bins (MG_PERCENTILE_WALK workgroups: beyond 8e12 elements).  One kernel launch; no
 * allocation, no synchronisation. */
int mg_percentile_histogram(const void* d_data, int dtype, int n0, int64_t stride0, int n1, int64_t stride1,
                            int64_t unit_len, int shift, int bits, int prefix_shift, const uint32_t* prefixes,
                            int n_prefixes, uint64_t* d_hist, void* stream);

/* The montage.  Window (g, c, t) of `dtype`, roi_len x roi_len contiguous, at d_roi + g * stride_m + c * stride_c + t *
 * stride_t (elements).  d_layout int32 [rows][cols] on the device: the marker of every cell, < 0 (or >= n_marks) for an
 * empty one.  d_out uint8 [n_t][rows * lk][cols * lk][3] with s = 2^level, lk = ceil(roi_len / s); every byte is
 * written once.  Per pixel of a cell: steps 1-4 of mg_render_overview on the window's s x s block (limits double
 * [n_c][2], colors double [n_c][3], host arrays); then the masks, bg with (255, 0, 0) first and fg with (0, 255, 0) on
 * top -- mask (g, t) is roi_len^2 bytes at d + g * stride_m + t * stride_t (0 is legal, as in mg_roi_image_labels), a
 * null mask is skipped; a block is on where any mask byte in it is non-zero; overlay 2 ("fill"): where on, acc = (1 -
 * alpha) * acc + (alpha * rgb) / 255; overlay 1 ("outline"): the same with alpha = 1, only where the block is on and
 * one of its four neighbours in the cell is off (outside the cell is off); overlay 0: none.  byte = floor(255 * acc +
 * 0.5); an empty cell is 0.  rows * cols = 0 is legal and launches nothing.  MG_EINVAL, with nothing launched: a null
 * roi / layout / output (where there are cells) / limits / colors, an unknown dtype, n_c outside 1 ..
 * MG_OVERVIEW_MAX_CHANNELS, n_t < 1, roi_len outside 1 .. 32767, level outside 0 .. MG_OVERVIEW_MAX_LEVEL, n_marks < 1
 * where there are cells, a negative count or stride, an unknown overlay, alpha or a colour outside [0, 1].  One kernel
 * launch; no allocation, no synchronisation. */
int mg_render_roi_montage(const void* d_roi, int dtype, int64_t stride_m, int64_t stride_c, int64_t stride_t, int n_marks,
                          int n_c, int n_t, int roi_len, int level, const int32_t* d_layout, int rows, int cols,
                          const double* limits, const double* colors, const uint8_t* d_bg, int64_t bg_stride_m,
                          int64_t bg_stride_t, const uint8_t* d_fg, int64_t fg_stride_m, int64_t fg_stride_t, int overlay,
                          double alpha, uint8_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------
 * Depth stacks (depth.py, the `project_depth` component; not in the reference, which refuses a Z axis; DESIGN.md
 * "Depth stacks"; tests/depth_ref.py restates every rule).  The input of all three entries is one contiguous block
 * (n, z, h, w) of `dtype`: n focal series (every channel x time x tile) of z slices.  The focus measure is the modified
 * Laplacian ML(y, x) = |2c - l - r| + |2c - u - d| of the pixel c and its left / right / upper / lower neighbours,
 * a neighbour outside the plane being the edge pixel (np.pad(mode="edge")).  Integer pixels: int32 arithmetic, exact.
 * Float pixels: float64, every operation rounded on its own, fabs((2 * c - l) - r) + fabs((2 * c - u) - d).
 * Every entry: MG_EINVAL, with nothing launched, for a null or misaligned pointer, an unknown dtype, n, h or w < 0,
 * h above 2^30 or w above 2^20 (the limits of all plane filters: csrc/mg_planes.h), z < 1; then MG_OK with nothing
 * launched (and nothing written) when n, h or w is 0 -- the arguments are judged first, so a misaligned pointer is
 * refused with an empty block too.  No allocation, no synchronisation.
 * ---------------------------------------------------------------------------------- */
#define MG_DEPTH_MAX 0
#define MG_DEPTH_MEAN 1
#define MG_DEPTH_PICK 2
#define MG_DEPTH_TILE 32  /* mg_depth_fuse: a workgroup's output tile is MG_DEPTH_TILE x MG_DEPTH_TILE pixels */
#define MG_DEPTH_MAX_K 15
#define MG_DEPTH_MAX_Z 255
#define MG_DEPTH_PROJECT_WALK 4096       /* mg_depth_project: workgroups over all stacks */
#define MG_DEPTH_FOCUS_WALK 4096         /* mg_depth_focus_totals: workgroups over all slices ... */
#define MG_DEPTH_FOCUS_WALK_PER_SLICE 64 /* ... and at most this many share a slice (one atomic each) */

/* d_dst (n, h, w) of `dtype` (a buffer other than d_src) = the fold of every stack over z.
 *   MG_DEPTH_MAX: m = slice 0; for z = 1, 2, ...: m = s where s > m; for floats a NaN in any slice gives NaN (the first
 *     one met), and of equal values (-0.0 and 0.0) the first stays.
 *   MG_DEPTH_MEAN: integer pixels: rint(sum / z) in float64 with the exact integer sum (half to even); float pixels: a
 *     float64 accumulator that starts at 0.0, slices added in the order z = 0, 1, ..., then / z, then the cast.
 *   MG_DEPTH_PICK: d_dst[i] = d_src[i, d_pick[i]]; d_pick is int32 (n) on the device (null otherwise).  The CALLER
 *     checks 0 <= d_pick[i] < z before the call (depth.project does); the kernel clamps what it reads, so that a bad
 *     index reads a wrong slice and no foreign memory.
 * One launch; every input byte is read once (PICK: the chosen slices only).  MG_EINVAL also for an unknown method and
 * a null d_pick with MG_DEPTH_PICK. */
int mg_depth_project(const void* d_src, void* d_dst, int dtype, int64_t n, int z, int h, int w, int method,
                     const int32_t* d_pick, void* stream);

/* d_totals (n, z), 8 bytes per entry, 8-byte aligned: the sum of ML over all pixels of slice (i, z) -- uint64 and exact
 * for MG_U8 / MG_U16, float64 for MG_F32 / MG_F64 (a sum of float64 terms in no defined order: compare by tolerance).
 * The entry zeroes d_totals itself; one 64-bit atomic per workgroup and slice. */
int mg_depth_focus_totals(const void* d_src, int dtype, int64_t n, int z, int h, int w, void* d_totals, void* stream);

/* The per-pixel pick of the sharpest slice, z <= MG_DEPTH_MAX_Z, window half-width 1 <= k <= MG_DEPTH_MAX_K.  The
 * measure of pixel (y, x) in a slice is the sum of ML over the (2k + 1)^2 window centred on it, window positions
 * outside the plane left out.  Integer pixels: uint32 sums, exact in any order (at most 4 * 65535 * 31^2 < 2^32).  Float
 * pixels: float64, in this order: per window row a sum that starts at 0.0 and adds the row's 2k + 1 values left to
 * right, then a sum that starts at 0.0 and adds the 2k + 1 row sums top to bottom (a position left out adds nothing).
 * The winner is found with best = -inf, winner = 0, and for z = 0, 1, ...: measure > best makes z the winner -- the
 * first of equal measures wins, an all-equal stack gives 0, a NaN measure never wins.  d_dst (n, h, w) of `dtype` (a
 * buffer other than d_src) receives the winner's pixel, d_index (n, h, w) uint8, if not null, its z.  One launch;
 * MG_EINVAL also for z > MG_DEPTH_MAX_Z and k outside 1 .. MG_DEPTH_MAX_K. */
int mg_depth_fuse(const void* d_src, int dtype, int64_t n, int z, int h, int w, int k, void* d_dst, uint8_t* d_index,
                  void* stream);

/* ------------------------------------------------------------------------------------
 * Hot pixels (despeckle.py, the `remove_outliers` component; not in the reference; DESIGN.md "Despeckle";
 * tests/despeckle_ref.py restates every rule).  The input of both entries is one contiguous block (n, h, w) of `dtype`:
 * n planes.  With the window half-width k (1 .. MG_DESPECKLE_MAX_K), the WINDOW MEDIAN m(y, x) of a plane P is the
 * middle element (index ((2k + 1)^2 - 1) / 2) of the ascending sort of the (2k + 1)^2 values P[clamp(y + dy, 0, h - 1),
 * clamp(x + dx, 0, w - 1)], |dy|, |dx| <= k: scipy.ndimage.median_filter(P, 2k + 1, mode="nearest").  It is one of
 * the window's pixels, exact in every dtype.  Floats sort as numpy.sort sorts them, every NaN after +inf: the median
 * is NaN only when more than half of the window is; -0.0 and 0.0 are not told apart (either may be returned).
 * The OUTLIER TEST of a pixel, with d = (double)P[y, x] - (double)m(y, x) and the threshold in pixel units:
 *   MG_OUTLIER_BRIGHT: d > threshold;  MG_OUTLIER_DARK: -d > threshold;  MG_OUTLIER_BOTH: either;
 *   MG_OUTLIER_ALL: always true (the plain median filter).
 * The inequality is strict (at threshold 0 a pixel equal to its median passes no test) and false whenever d is NaN
 * (a NaN pixel, a NaN median, inf - inf): such a pixel is kept.
 * Both entries: MG_EINVAL, with nothing launched, for a null or misaligned pointer, an unknown dtype or `which`, n, h
 * or w < 0, h above 2^30 or w above 2^20, k outside 1 .. MG_DESPECKLE_MAX_K, a negative or NaN threshold where it is used;
 * then MG_OK with nothing launched (and nothing written) when n, h or w is 0 -- the arguments are judged first, so a
 * misaligned pointer is refused with an empty block too (csrc/mg_planes.h).  A workgroup takes one MG_DESPECKLE_TILE x
 * MG_DESPECKLE_TILE output tile of a plane at a time, the tile and its halo of k in LDS; the plane index is not bounded by a grid
 * dimension and every offset into the block is 64-bit.  One kernel launch behind the clearing of the counters; no
 * allocation, no synchronisation.
 * ---------------------------------------------------------------------------------- */
#define MG_OUTLIER_BRIGHT 0
#define MG_OUTLIER_DARK 1
#define MG_OUTLIER_BOTH 2
#define MG_OUTLIER_ALL 3
#define MG_DESPECKLE_MAX_K 2
#define MG_DESPECKLE_TILE 64  /* a workgroup's output tile is MG_DESPECKLE_TILE x MG_DESPECKLE_TILE pixels */
#define MG_DESPECKLE_WALK 2048 /* workgroups over all planes */

/* d_dst (n, h, w) of `dtype` (a buffer other than d_src): d_dst[i, y, x] = m(y, x) of plane i where the CONDITION holds,
 * else d_src[i, y, x] bit for bit.  The condition is the outlier test `which` with `threshold`, or, with a defect map
 * d_defects (uint8 (h, w), shared by all planes; may be null), d_defects[y, x] != 0 -- `which` (still a known one) and
 * `threshold` are then ignored, as `threshold` is with MG_OUTLIER_ALL.  d_counts (n) int64, 8-byte aligned, may be
 * null: the number of pixels of every plane for which the condition held; the entry zeroes it itself, one 64-bit
 * integer atomic per workgroup and plane (integers: exact in any order). */
int mg_despeckle_planes(const void* d_src, void* d_dst, int dtype, int64_t n, int h, int w, int k, int which,
                        double threshold, const uint8_t* d_defects, int64_t* d_counts, void* stream);

/* d_votes (h, w) int32: the number of the n planes in which pixel (y, x) passes the outlier test (BRIGHT, DARK or
 * BOTH; MG_EINVAL for MG_OUTLIER_ALL).  The entry zeroes d_votes itself; one int32 atomic per pixel that passes, so the
 * table is exact in any order.  n > 2^31 - 1 is MG_EINVAL (a vote count is int32). */
int mg_outlier_votes(const void* d_src, int dtype, int64_t n, int h, int w, int k, int which, double threshold,
                     int32_t* d_votes, void* stream);

/* ------------------------------------------------------------------------------------
 * Background (background.py, the `subtract_background` component; not in the reference; DESIGN.md "Background";
 * tests/background_ref.py restates every rule).  The input is one contiguous block (n, h, w) of `dtype`: n planes P.
 * With the radius R (1 .. MG_BACKGROUND_MAX_RADIUS) the WINDOW of a pixel is the (2R + 1) x (2R + 1) square centred on
 * it; window positions outside the plane are left out, and so are NaN pixels; a window with nothing left gives NaN.
 *   EROSION   E(y, x) = the minimum of F over the window;
 *   OPENING   B(y, x) = the maximum of E over the window -- the background: what is left of the plane when everything
 *             narrower than the window is taken away.
 * F is the FILTERED plane: d_filtered, a block like d_src (mg_despeckle_planes with MG_OUTLIER_ALL makes one), or, where
 * d_filtered is null, P itself.  On planes without NaN, B is scipy.ndimage.grey_opening(F, size=2R + 1, mode="nearest"),
 * bit for bit.  Every value of E and B is one of F's: exact in every dtype; -0.0 and 0.0 are not told apart (either
 * may be returned).
 *   MG_BACKGROUND_ESTIMATE: d_dst = B.
 *   MG_BACKGROUND_SUBTRACT: d_dst = P - B where P > B, else 0, computed in `dtype`; NaN where P or B is NaN.  With
 *     F = P, B <= P everywhere; with a filtered F it is not, and the clamp at 0 is part of the rule.
 * Minimum and maximum over a square are separable: the opening is min-x, min-y, max-y, max-x, each a 1-D pass over
 * blocks of 2R + 1 with running extrema from either end (van Herk / Gil-Werman), about three compares per pixel
 * whatever R.  Three launches -- the two vertical passes are one kernel, which takes up to MG_BACKGROUND_COLS columns
 * (fewer where the rows it needs, MG_BACKGROUND_ROWS + 4R, would not fit in LDS) and MG_BACKGROUND_ROWS rows at a time;
 * the horizontal kernels take MG_BACKGROUND_SPAN columns of up to 64 rows at a time.  Four reads and three writes of
 * a block in all.  The plane index is not bounded by a grid dimension and every offset into the block is 64-bit.
 * mg_background_planes: MG_EINVAL, with nothing launched, for a null or misaligned pointer (d_filtered may be null),
 * an unknown dtype or mode, n, h or w < 0, h above 2^30 or w above 2^20, R outside 1 .. MG_BACKGROUND_MAX_RADIUS,
 * scratch_bytes below mg_background_scratch_bytes of the same sizes, d_dst or d_scratch equal to another buffer; MG_OK
 * with nothing launched (and nothing written) when n, h or w is 0.  No allocation, no synchronisation.
 * ---------------------------------------------------------------------------------- */
#define MG_BACKGROUND_ESTIMATE 0
#define MG_BACKGROUND_SUBTRACT 1
#define MG_BACKGROUND_MAX_RADIUS 128
#define MG_BACKGROUND_ROWS 128  /* the vertical kernel: output rows of a workgroup's step */
#define MG_BACKGROUND_COLS 64   /* the vertical kernel: columns of a workgroup's step, at most */
#define MG_BACKGROUND_SPAN 256  /* the horizontal kernels: output columns of a workgroup's step */
#define MG_BACKGROUND_WALK 16384 /* workgroups of one pass */

/* The bytes of d_scratch that mg_background_planes needs for these sizes (two blocks (n, h, w) of `dtype`; 0 for an
 * empty block), or -1 where it would refuse them. */
int64_t mg_background_scratch_bytes(int dtype, int64_t n, int h, int w, int radius);

/* d_dst (n, h, w) of `dtype` = B (MG_BACKGROUND_ESTIMATE) or the clamped P - B (MG_BACKGROUND_SUBTRACT) of every plane
 * of d_src; d_scratch: scratch_bytes bytes on the device, aligned like the planes, contents undefined afterwards. */
int mg_background_planes(const void* d_src, const void* d_filtered, void* d_dst, int dtype, int64_t n, int h, int w,
                         int radius, int mode, void* d_scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Skew (skew.py, `rotate(rotation="auto")`; not in the reference; tests/skew_ref.py restates every
 * rule): the projection profiles of one plane along every angle of a table, in integers only -- the same bits in any
 * order.  d_plane: (h, w) of `dtype`, row y at d_plane + y * row_stride elements.  With D = min(h, w) and
 * nb = D + 2, d_sums (uint64) and d_counts (uint32) are contiguous (n_angles, 2, nb), ZEROED BY THE CALLER; axis 0 is
 * the row profile, axis 1 the column profile.
 *   QUANTISED PIXEL q.  MG_U8 / MG_U16: q = p.  MG_F32 / MG_F64: a NaN pixel is left out of sums and counts; otherwise
 *     t = (p - lo) * scale in float64 (two roundings, no fused multiply-add), q = 0 where t < 0, 65535 where t > 65535,
 *     else floor(t) (a NaN t, which only an infinite pixel can give, counts as 0).  lo and scale are not read for
 *     integer pixels, but are checked.
 *   GEOMETRY.  dy = 2 y - (h - 1), dx = 2 x - (w - 1); a pixel takes part iff dy^2 + dx^2 <= (D - 1)^2 (the inscribed
 *     disk: the length of a projection line does not depend on the angle).  d_cs[a] = (C, S) =
 *     (rint(32768 cos), rint(32768 sin)) of angle a, built by the caller;
 *     kr = ((dy C - dx S) >> 16) + nb / 2,  kc = ((dx C + dy S) >> 16) + nb / 2   (int64 products, arithmetic shift);
 *     sums[a, 0, kr] += q, counts[a, 0, kr] += 1, sums[a, 1, kc] += q, counts[a, 1, kc] += 1.
 *     With such a table both indices lie in [0, nb); an index that a table of other numbers puts outside is dropped.
 * A workgroup takes one MG_SKEW_TILE x MG_SKEW_TILE tile at a time, reads it once, and walks the whole table over it:
 * the plane is read from memory once per call.  A tile's partial sums are 32-bit (MG_SKEW_TILE^2 * 65535 < 2^32), held
 * in LDS, and reach d_sums / d_counts as 64- / 32-bit integer atomics, non-empty bins only.
 * MG_EINVAL, with nothing launched: a null or misaligned pointer, an unknown dtype, h or w outside 8 .. MG_SKEW_MAX_SIDE,
 * row_stride < w, n_angles outside 1 .. MG_SKEW_MAX_ANGLES, a non-finite lo or scale.  One kernel launch; no
 * allocation, no synchronisation.
 * ---------------------------------------------------------------------------------- */
#define MG_SKEW_TILE 64
#define MG_SKEW_MAX_ANGLES 64
#define MG_SKEW_MAX_SIDE 32768
#define MG_SKEW_WALK 2048 /* workgroups; each walks its share of the plane's tiles */
int mg_skew_profiles(const void* d_plane, int dtype, int h, int w, int64_t row_stride, double lo, double scale,
                     const int32_t* d_cs, int n_angles, uint64_t* d_sums, uint32_t* d_counts, void* stream);

/* ------------------------------------------------------------------------------------
 * Blobs (blobs.py, `find_blobs`; not in the reference; tests/blobs_ref.py restates every rule):
 * connected components of a thresholded plane as markers of any shape.  Integer arithmetic only; every output is the
 * same bits from call to call.
 *
 * mg_blob_labels.  d_plane: one contiguous (h, w) plane of `dtype`.  A pixel v is ON iff (double)v > threshold, with
 *   `below` iff (double)v < threshold; NaN is never on.  connectivity is 4 or 8.
 *   d_labels int32 (h, w): -1 where off, else the component's number 0 .. K-1; components are numbered in raster order
 *     of their first pixel (smallest y * w + x), the order of scipy.ndimage.label.
 *   d_num int32: K.
 *   d_stats int64 [cap][8] = {area, sum_y, sum_x, y_min, x_min, y_max, x_max, first_pixel}; rows 0 .. min(K, cap) - 1
 *     are written, the others are left alone.
 *   d_status int32: 0, or MG_BLOB_OVERFLOW (K > cap: d_num holds K, d_labels is complete, d_stats holds the first cap
 *     components) | MG_BLOB_EBOUND (a bounded loop ran out: an internal error, no output is to be trusted).
 *   d_scratch: mg_blob_scratch_bytes(h, w, cap) bytes owned by the caller, 16-byte aligned; its contents before the call
 *     do not matter, and d_num / d_status are re-initialised by the call: a call after a larger plane, or after a call
 *     that overflowed, is correct.
 *   Launches (no workgroup ever waits for another): clear; tile pass (one workgroup labels a MG_BLOB_TILE_H x
 *   MG_BLOB_TILE_W tile in LDS and writes, per on pixel, the linear index of the smallest pixel of its component inside
 *   the tile); seam pass (unions across the tile borders on that parent array, agent-scope atomics only); compress and
 *   count roots; one-workgroup scan of the counts; number the roots; flatten and statistics.  Every grid is sized by the
 *   tile / pixel count, none is capped.
 *   MG_EINVAL, with nothing launched: a null pointer, an unknown dtype, h or w < 1, h * w beyond int32, a
 *   connectivity other than 4 or 8, cap < 1, a NaN threshold, scratch_bytes below mg_blob_scratch_bytes, a misaligned
 *   d_scratch or d_stats.  No allocation, no synchronisation.
 *
 * mg_blob_select.  Component k < K = min(*d_num, cap) is kept iff min_area <= area, area <= max_area where
 *   max_area > 0, and, with clear_border, y_min > 0, x_min > 0, y_max < h - 1 and x_max < w - 1.  The kept components
 *   are renumbered 0 .. M-1 in their order; d_labels is rewritten in place (kept: the new number, rejected: -2,
 *   off: -1).  d_num_kept int32: M.  d_stats_out int64 [cap][8]: the kept rows, compacted (must not overlap d_stats).
 *   d_table int32 [cap][3] = {row, col, r}: row = floor((2 sum_y + area) / (2 area)), col likewise from sum_x, and
 *   r = the largest integer with 355 (2 r - 1)^2 <= 452 area: the nearest integer to sqrt(area / pi) with pi taken as
 *   355 / 113.  d_remap int32 [cap]: workspace.  Two launches.  MG_EINVAL: null pointers, h, w as above, cap < 1,
 *   negative areas.
 *
 * mg_blob_fill_holes.  d_clabels / d_cstats: labels and statistics of the COMPLEMENT of the mask (mg_blob_labels with
 *   connectivity 4 and the opposite polarity).  Every pixel of a complement component whose bounding box touches no side
 *   of the frame is set to 1 in d_on u8 (h, w): scipy.ndimage.binary_fill_holes with its default structure.  One launch.
 *   d_cstats has `cap` rows (the complement's component count, or fewer): a pixel whose number is >= cap is left alone,
 *   no row beyond cap is read.  MG_EINVAL, with nothing launched: a null pointer, h or w < 1, h * w beyond int32,
 *   cap < 1.
 *
 * mg_blob_threshold.  The on mask of mg_blob_labels alone, for the same plane, threshold and `below`: d_on u8 (h, w),
 *   1 where on, 0 where off.  One launch.  MG_EINVAL, with nothing launched: a null or misaligned pointer, an unknown
 *   dtype, h or w < 1, h * w beyond int32, a NaN threshold.
 * ---------------------------------------------------------------------------------- */
#define MG_BLOB_TILE_H 32
#define MG_BLOB_TILE_W 64
#define MG_BLOB_OVERFLOW 1
#define MG_BLOB_EBOUND 2
int64_t mg_blob_scratch_bytes(int h, int w, int64_t cap);
int mg_blob_labels(const void* d_plane, int dtype, int h, int w, double threshold, int below, int connectivity,
                   int32_t* d_labels, int32_t* d_num, int64_t* d_stats, int64_t cap, int32_t* d_status, void* d_scratch,
                   int64_t scratch_bytes, void* stream);
int mg_blob_threshold(const void* d_plane, int dtype, int h, int w, double threshold, int below, uint8_t* d_on,
                      void* stream);
int mg_blob_select(int32_t* d_labels, int h, int w, const int64_t* d_stats, const int32_t* d_num, int64_t cap,
                   int64_t min_area, int64_t max_area, int clear_border, int32_t* d_num_kept, int64_t* d_stats_out,
                   int32_t* d_table, int32_t* d_remap, void* stream);
int mg_blob_fill_holes(const int32_t* d_clabels, const int64_t* d_cstats, int64_t cap, int h, int w, uint8_t* d_on,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAGNIFY_HIP_H */
