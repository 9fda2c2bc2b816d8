/*
 * treelearn_hip.h -- C ABI of libtreelearn_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary of the TreeLearn per-tile sparse-conv segmentation path.  The
 * reference (ecker-lab/TreeLearn) has no FFI of its own: its device work is delegated to
 * the third-party `spconv` wheel and to ATen.  Each entry point below replaces one of
 * those call sites (cited as reference file:line).  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (the PyTorch-ROCm caching
 *     allocator in our host code); the library never allocates or frees device memory;
 *   - every call takes the hipStream_t to enqueue on (as void*) and returns immediately;
 *   - return value: 0 = TL_OK, negative = error (tl_error_string); no exceptions; the only
 *     process-wide state is the set of developer switches behind tl_set_tuning (kernel-family
 *     selection for A/B runs and tests; results do not depend on them beyond re-association);
 *     calls on one stream must not be issued concurrently;
 *   - "table" = rulebook in tap-major layout i32[K][n_out], entry = input row or -1
 *     (SURVEY.md Appendix F canonical form, transposed for coalesced access).
 */
#ifndef TREELEARN_HIP_H
#define TREELEARN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tl_stream_t; /* hipStream_t */

enum {
  TL_OK = 0,
  TL_ERR_ARG = -1,       /* bad argument (null pointer, unsupported size) */
  TL_ERR_LAUNCH = -2,    /* hipGetLastError() after a launch was not hipSuccess */
  TL_ERR_UNSUPPORTED = -3
};

/* TL_F16 (IEEE half, BASELINE config 5's "fp16"; the reference trains under fp16 autocast + GradScaler, tools/training/train.py:32,40-44):
 * served by every entry point that takes a dtype -- the conv / head / weight-packing path and, since round 5, the training entry points
 * (tl_conv_wgrad*, tl_bn_train_*, the epilogue modes of tl_conv_fwd, tl_gather_rows / tl_scatter_add_rows, tl_linear_small_f32): the units are
 * compiled a second time for _Float16 (csrc/tl_half.h, tl_f16_train.h).  One 16-bit type per call (no bf16 / f16 mixtures).  Values beyond
 * 65504 become inf (no saturation), as on any fp16 path. */
enum { TL_F32 = 0, TL_BF16 = 1, TL_F16 = 2 };

int tl_version(void);
/* Developer tuning knobs, process-wide.  Kernel families and forms, 1 = on (default), 0 = off: "direct" / "stream" / "streamq" /
 * "blk" (the staged-unit kernel of the block-local level) / "up" (the scatter form of the inverse conv) / "direct_oh" (the gather-once
 * form of the level-1 inverse conv) / "streamq_x3" (the quad-gather kernel for fp32 rows in the bf16x3 mode; 0 or 1 only).  Row
 * thresholds: "small_rows", "wgrad_dense_min_rows".  Variants: "small_mode" (small-level conv kernel), "wgrad_dense" / "wgrad_rows" /
 * "wgrad_dma" (weight-gradient kernels).  Any other key returns TL_ERR_ARG.  Not needed for correct results; the parity tests use them
 * to force every family over the same data.  They are read on the host when a launch is
 * dispatched (launches already enqueued are unaffected); do not change them while another host thread is inside the library. */
int tl_set_tuning(const char* key, int64_t value);
const char* tl_error_string(int code);

/* ------------------------------------------------------------------ voxel hashing
 * Replaces spconv PointToVoxel.generate_voxel_with_id + the min/max/.tolist() prologue of
 * `voxelize` (reference tree_learn/model/tree_learn.py:129-167, call site :136-143).
 *
 * The "hash table" is a succinct rank structure instead of an open-addressing table:
 * an occupancy bitmap over the tile's voxel grid (1 bit per cell, z along the 64-bit word)
 * plus an exclusive prefix sum of word popcounts.  rank(cell) = prefix[word] +
 * popc(word & below(bit)) is the voxel's row in ascending (b,x,y,z) order, i.e. the
 * canonical order of SURVEY.md Appendix F, with no sort and no probing.
 */

/* Per-point integer voxel coordinates.
 *   xyz f32[N,3], batch_ids i64[N], B batch elements, voxel_size.
 *   ws_minmax u32[B*6] scratch; pcoords i32[N,4] out = (b,x,y,z) with
 *   x = floorf((p - min_b) / voxel_size) in fp32 (tree_learn.py:134, spconv PointToVoxel);
 *   maxc i32[4] out = {max x, max y, max z, error flag}. */
int tl_voxel_point_coords(const float* xyz, const int64_t* batch_ids, int64_t N, int B, float voxel_size,
                          uint32_t* ws_minmax, int32_t* pcoords, int32_t* maxc, tl_stream_t stream);

/* Occupancy bitmap of the level-1 grid.  dims = {B, X, Y, Z}; bitmap u64[B*X*Y*ceil(Z/64)] (zeroed here). */
/* The same for ONE tile (B = 1, what the tile loop's forward passes: tree_learn/util/pipeline.py:83-88), without same-address atomics: the
 * per-workgroup coordinate maxima are written as rows of `maxc_parts` i32[TL_POINT_COORDS_MAX_PARTS][4] = (max x, max y, max z, error
 * flag); *n_parts (host) rows are valid and the caller folds them (max / or) after its read-back.  ws: u32[6 * 256].  pcoords as above. */
#define TL_POINT_COORDS_MAX_PARTS 1024
int tl_voxel_point_coords_one(const float* xyz, const int64_t* batch_ids, int64_t N, float voxel_size, uint32_t* ws, int32_t* pcoords,
                              int32_t* maxc_parts, int* n_parts, tl_stream_t stream);
int tl_bitmap_from_points(const int32_t* pcoords, int64_t N, const int32_t dims[4], uint64_t* bitmap, tl_stream_t stream);

/* Occupancy of the stride-2 coarse grid (SparseConv3d k=2 s=2 output set, reference
 * tree_learn/model/blocks.py:104-110): coarse cell = OR of its 2x2x2 children; cells at or beyond
 * out_shape[3] (= in_shape // 2) are dropped.
 * fdims = {B,Xf,Yf,Zf}; cdims = {B, ceil(Xf/2), ceil(Yf/2), ceil(Zf/2)}. */
int tl_bitmap_down(const uint64_t* fine, const int32_t fdims[4], const int32_t out_shape[3],
                   uint64_t* coarse, const int32_t cdims[4], tl_stream_t stream);

/* Exclusive prefix sum of popcounts.  prefix u32[nwords]; total u32[1] (device); ws u32[tl_scan_ws_words(nwords)]. */
int64_t tl_scan_ws_words(int64_t nwords);
int tl_bitmap_scan(const uint64_t* bitmap, int64_t nwords, uint32_t* prefix, uint32_t* total, uint32_t* ws, tl_stream_t stream);

/* coords i32[M,4] = (b,x,y,z) of every set bit, in rank order. */
int tl_expand_coords(const uint64_t* bitmap, const uint32_t* prefix, const int32_t dims[4], int32_t* coords, tl_stream_t stream);

/* v2p i64[N]: voxel row of every point (tree_learn.py:143 pc_voxel_id, :160-161 batch offsets implicit). */
int tl_point_rank(const int32_t* pcoords, int64_t N, const uint64_t* bitmap, const uint32_t* prefix,
                  const int32_t dims[4], int64_t* v2p, tl_stream_t stream);

/* Optional voxel features (use_coords / use_feats, tree_learn.py:149-156): mean over the first <= P points of
 * each voxel in input order, all-zero point rows skipped; pf f32[N,C] rows (x,y,z,feat..); out f32[M,C]
 * in (x,y,z,feat..) order; ws i32[M*P] scratch. */
int tl_voxel_mean_feats(const float* pf, int C, const int64_t* v2p, int64_t N, int64_t M, int P,
                        int32_t* ws, float* out, tl_stream_t stream);
/* The same means straight into the input conv's operand (tree_learn.py:149-156 in one launch sequence): columns (x, y, z) from
 * xyz f32[N,3] and f_0..f_{F-1} from feats f32[N,F] (F <= 5), column groups switched off by use_coords / use_feats = 0 set to 1,
 * output rows in the reference's (feat.., x, y, z) order, cast to `dtype` (round to nearest even): out [M, 3 + F]; ws i32[M*P]. */
int tl_voxel_feats(const float* xyz, const float* feats, int F, const int64_t* v2p, int64_t N, int64_t M, int P, int use_coords,
                   int use_feats, int dtype, int32_t* ws, void* out, tl_stream_t stream);

/* ------------------------------------------------------------------ rulebooks
 * Replaces spconv's indice generation for SubMConv3d(k=3,pad=1) (`subm{l}`, tree_learn.py:37-39,
 * blocks.py:57-70) and SparseConv3d(k=2,s=2)/SparseInverseConv3d(k=2) (`spconv{l}`, blocks.py:104-123). */

/* nbr i32[27][M]: tap = (dx+1)*9 + (dy+1)*3 + (dz+1), entry = input row or -1; nbr[13][i] == i. */
int tl_rulebook_subm(const int32_t* coords, int64_t M, const uint64_t* bitmap, const uint32_t* prefix,
                     const int32_t dims[4], int32_t* nbr, int32_t* compact /* optional i32[10][M] column form, see tl_rulebook_compact */,
                     tl_stream_t stream);

/* child i32[8][Mc] (tap = (x&1)*4+(y&1)*2+(z&1)), parent i32[Mf] (-1 = dropped), inv i32[8][Mf]
 * (inv[tap(p)][p] = parent[p], other taps -1: the inverse conv's table).  parent and inv are filled here. */
int tl_rulebook_down(const int32_t* ccoords, int64_t Mc, const uint64_t* fbitmap, const uint32_t* fprefix,
                     const int32_t fdims[4], int64_t Mf, int32_t* child, int32_t* parent, int32_t* inv, tl_stream_t stream);

/* ---- the whole pyramid in two calls (what treelearn_amd.geometry uses; same kernels and results as the per-level calls
 * above, enqueued back to back, the deep levels -- a few thousand words each -- batched into shared launches).
 *
 * tl_pyramid_ws_words: scratch (u32 words: the scans' partial sums + a byte map of level 1, 64 B per bitmap word) for a pyramid whose level 1
 *   has dims0 = {B,X,Y,Z}; level l+1 has
 *   ceil(dims_l / 2).  level_word_offsets (optional, i64[num_levels+1]) receives the word offset of every level inside the
 *   `bitmaps` / `prefixes` arrays (the last entry = total words).
 * tl_pyramid_build: occupancy bitmap of level 1 from pcoords, then per level the k2s2 down-sampling (cells at or beyond
 *   shape_l = shape0 >> l dropped, spconv's floor((n-2)/2)+1 output shape; tree_learn.py:86-87, blocks.py:104-108) and the
 *   popcount scan; counts u32[num_levels] (device) = active voxels per level. */
int64_t tl_pyramid_ws_words(const int32_t dims0[4], int num_levels, int64_t* level_word_offsets);
int tl_pyramid_build(const int32_t* pcoords, int64_t N, const int32_t dims0[4], const int32_t shape0[3], int num_levels,
                     uint64_t* bitmaps, uint32_t* prefixes, uint32_t* counts, uint32_t* ws, tl_stream_t stream);

/* One level of the pyramid for tl_rulebooks_build: inputs dims/n/bitmap/prefix, outputs as in tl_expand_coords,
 * tl_rulebook_subm (nbr, optional compact) and tl_rulebook_down (child/parent/inv: the tables between this level and the
 * next coarser one; unused on the last level). */
typedef struct tl_level {
  int32_t dims[4];
  int64_t n;
  const uint64_t* bitmap;
  const uint32_t* prefix;
  int32_t* coords;
  int32_t* nbr;
  int32_t* compact;
  int32_t* child;
  int32_t* parent;
  int32_t* inv;
  /* optional (NULL = canonical order): the block-local order of THIS level (tl_blk_build's o2n).  The tables that hold or are indexed
   * by rows of this level -- child (entries), parent / inv (index) and, on level 1, v2p (entries) -- are then written in that order.
   * With o2n set, coords / nbr / compact of the level may be NULL (the block-local conv kernel needs none of them). */
  const int32_t* o2n;
  /* optional: the inverse table of this level in its packed form i32[n] = (parent row << 3) | tap, -1 = no parent -- 4 B per row instead of the
   * 32 B of the one-hot `inv` (tl_conv_args.table_one_hot = 2 reads it).  With inv_packed set, `inv` may be NULL; `parent` may always be NULL. */
  int32_t* inv_packed;
} tl_level;

/* coords + every rulebook of every level + (v2p != NULL) the point -> voxel map, in one call.  parent / inv arrays that lie
 * inside [minus_one, minus_one + minus_one_words) are set to -1 by a single fill of that block (optional; others are filled
 * one by one). */
int tl_rulebooks_build(const tl_level* levels, int num_levels, int32_t* minus_one, int64_t minus_one_words,
                       const int32_t* pcoords, int64_t N, int64_t* v2p, tl_stream_t stream);

/* ---- block-local row order + staged rulebook of a level (what the level-1 convs of the inference engine run on; csrc/tl_blk.hip).
 * The reference's spconv keeps voxels in hash order and gathers every tap of every output row (blocks.py:57-70 -> spconv's
 * implicit-GEMM gather); the canonical order here (ascending key) pins the bit-exact rulebook tests.  For the matrix-core kernel a
 * THIRD, internal order is better: voxels sorted by 8x8x8 block -- blocks ordered by (batch, x >> 5, y >> 5, (x >> 3) & 3, (y >> 3) & 3,
 * z >> 3), i.e. tiles of 4 x 4 block columns --, canonical order inside a block.  Units of <= 64
 * consecutive rows of that order then reach few rows outside themselves (their "halo"), so a wave can stage own + halo rows once in
 * LDS and read all 27 taps from there.
 *   o2n / perm     i32[n]: canonical row -> new row and back;  coords_new i32[n][4] = (b,x,y,z) in the new order
 *   unit           i32[cap_units][4] = {first new row, rows (1..64), halo rows, 0}.  Chunk c = new rows [64 c, 64 c + 64) is unit c when
 *                  its halo has <= halo_max rows; otherwise it is halved (recursively) and the pieces after the first are appended
 *                  behind the ceil(n / 64) regular units, ascending by first row.  counter[0] (DEVICE) = number of units, counter[1] = error flag
 *   halo           i32[32 n]: the unit that starts at row r0 lists its DISTINCT outside rows ascending at halo + 32 r0, padded with -1
 *                  to a multiple of 16
 *   lrb            u32[n][9]: 27 ten-bit entries per row, tap k in word k / 3 at bits 10 (k % 3): entry = 4 * pos + ((pos >> 2) & 3), so that
 *                  entry * 16 is the byte offset of tap k's input row in the unit's stage (64-B rows, 16-B pieces XOR-swizzled), with
 *                  pos = own row index (0..63), 64 + halo rank, or 191 = absent (the stage's zero row)
 *   pmask          i32[n]: 27-bit presence mask of the row's taps
 * n < 2^25.  ws u32[tl_blk_ws_words(dims)] (16-B aligned).  Deterministic: the appended units are sorted by their first row. */
#define TL_BLK_HALO_MAX 126
typedef struct tl_blk {
  int32_t* o2n; int32_t* perm; int32_t* coords_new;
  int32_t* unit; int32_t* counter; int32_t* halo; uint32_t* lrb; int32_t* pmask;
  int64_t cap_units;        /* rows of `unit` (>= ceil(n / 64); n always suffices) */
  int32_t halo_max;         /* 26 .. TL_BLK_HALO_MAX */
  int32_t reserved;
  int32_t* nn;              /* optional (NULL = not wanted): the rulebook as a plain table i32[27][n] in the NEW row order (entry = new input row or
                             * -1) -- what the kernels without a staged form read (weight gradient, convs of other widths) */
} tl_blk;
int64_t tl_blk_ws_words(const int32_t dims[4]);
/* phases: 1 = the order (o2n, perm, coords_new + the scratch the second phase reads), 2 = units / halo / lrb / pmask, 3 = both.  The
 * two phases may be enqueued on different streams (phase 2 after phase 1): what tl_rulebooks_build needs of a blocked level is o2n only,
 * so the unit builder -- instruction-bound, light on memory -- can run beside the rulebook kernels of the other levels. */
int tl_blk_build(const uint64_t* bitmap, const uint32_t* prefix, const int32_t dims[4], int64_t n, const tl_blk* out, uint32_t* ws,
                 int phases, tl_stream_t stream);

/* Column form of a 27-tap SubM rulebook built by tl_rulebook_subm: compact i32[10][n] = the row of the first present
 * dz neighbour of each of the 9 (dx, dy) columns (or -1) followed by a 27-bit presence mask.  Present neighbours of a
 * column are consecutive rows, so entry k = 3 c + d is compact[c] + popcount(mask bits 3c .. k-1).  tl_conv_fwd reads this
 * (40 B per voxel) instead of the table (108 B) in the kernels that support it (tl_conv_args.table_compact). */
int tl_rulebook_compact(const int32_t* table, int64_t n, int32_t* compact, tl_stream_t stream);

/* ------------------------------------------------------------------ sparse convolution
 * Replaces spconv SubMConv3d / SparseConv3d / SparseInverseConv3d forward (blocks.py:57-70,104-123,
 * tree_learn.py:37-39) and Custom1x1Subm3d's torch.mm (blocks.py:29-39), with the surrounding
 * BatchNorm1d+ReLU (blocks.py:56,63,103,117; tree_learn.py:42), residual add (blocks.py:76) and skip
 * concat (blocks.py:146, via in_ld/out_ld column views) fused as prologue / epilogue.
 *
 *   out[o, :] = epi( sum_k  W[k] . pro(in[table[k][o], :]) )        (absent rows contribute 0)
 *   pro(x) = relu?(x * in_scale + in_shift)       epi(y) = relu?((y + residual[o]) * out_scale + out_shift)
 *   out2 / out3 (optional) = relu?((y + residual[o]) * out{2,3}_scale + out{2,3}_shift)
 */
typedef struct tl_conv_args {
  const void* in;        int64_t in_ld;   /* row stride in elements (>= Cin) */
  const void* weight;                     /* [K][Cout][Cin], same dtype as `in` */
  const int32_t* table;                   /* [K][n_out], or NULL = identity (K must be 1) */
  int64_t n_out;         int64_t n_in;
  int32_t K;             int32_t Cin;     int32_t Cout;   int32_t dtype;   /* TL_F32 | TL_BF16 | TL_F16 */
  const float* in_scale; const float* in_shift;  int32_t in_relu;  int32_t out_relu;
  const void* residual;  int64_t res_ld;
  const float* out_scale; const float* out_shift;
  void* out;             int64_t out_ld;
  /* up to two extra views of y = acc + residual, each with its own affine/ReLU -- lets a producer store the
   * raw tensor (for the residual branch) AND relu(bn_next(y)) (for the next conv's gathers) in one pass: */
  void* out2; int64_t out2_ld; const float* out2_scale; const float* out2_shift; int32_t out2_relu;
  void* out3; int64_t out3_ld; const float* out3_scale; const float* out3_shift; int32_t out3_relu;
  /* optional second copy of the weights in MFMA-fragment order (tl_pack_weight_frag), NULL if absent: kernels that
   * read B operands straight from global memory (the small-level kernel) then load 1 KB contiguous per instruction */
  const void* weight_frag;
  /* != 0: every output row has at most ONE valid table entry (SparseInverseConv3d: the row's parent through its own
   * octant tap).  Kernels may then gather that single row once and route it to its tap instead of issuing K gathers.
   * 2: `table` is the PACKED form i32[n_out] = (input row << 3) | tap, -1 = none (tl_level.inv_packed; K = 8) -- served by the gather-once
   * kernels only (16-bit and bf16x3, 64 -> 32): any other shape returns TL_ERR_UNSUPPORTED rather than misreading the table. */
  int32_t table_one_hot;
  /* optional column form of `table` (tl_rulebook_compact; K must be 27), NULL if absent */
  const int32_t* table_compact;
  /* Training-mode epilogue reductions (the BatchNorm1d that surrounds every conv of the reference, blocks.py:55-70,102-123, in
   * train() mode; tools/training/train.py:30-44).  With y = acc + residual:
   *   TL_EPI_STATS : red_part f64[parts][2][Cout] receives per-workgroup sums of y and y^2 (y as stored) -- the batch statistics of
   *                  the BatchNorm that consumes this conv's output (finish: tl_bn_train_finish), without a pass over y;
   *   TL_EPI_BN_BWD: this launch is the input-gradient conv of a layer whose input was relu?(bn(x)): y is dy of that activation;
   *                  every view receives g = dy * [x * bn_scale + bn_shift > 0] (bn_relu) and red_part the sums of g and of
   *                  g * (x - bn_mean) * bn_rstd = dbeta / dgamma (finish + dx: tl_bn_train_bwd_from_parts).  bn_x [n_out, Cout]
   *                  in `dtype`, row stride bn_x_ld.
   * red_part must hold tl_conv_red_parts(n_out) rows; *red_nparts (HOST, optional) receives the rows actually written.
   * Only the direct / stream kernel families carry these epilogues: other shapes return TL_ERR_UNSUPPORTED (nothing launched)
   * and the caller runs the separate passes (tl_bn_train_stats / tl_bn_train_bwd).  Deterministic. */
  /* != 0: every element of `in` is 1 (the reference's default use_feats = False, use_coords = False feeds all-ones voxel features,
   * tree_learn.py:129-167): out[o] = sum over the present taps of sum_c W[k][:][c].  Served without reading `in` when K = 27,
   * Cout = 32, bf16 and table_compact is given; otherwise the flag is ignored (the general kernels read the ones). */
  int32_t in_all_ones;
  int32_t epi_mode;
  double* red_part;
  int32_t* red_nparts;
  const void* bn_x;      int64_t bn_x_ld;
  const float* bn_mean;  const float* bn_rstd;  const float* bn_scale;  const float* bn_shift;  int32_t bn_relu;
  /* Block-local form of a 27-tap SubM rulebook (tl_blk_build; all five NULL when absent).  `in`, `out*`, `residual` are then in the
   * block-local row order, `table` may be NULL, and K = 27, Cin = Cout = 32, TL_BF16 / TL_F16 are served by the staged-unit kernel
   * (csrc/tl_conv_blk.hip; same summation order as the gather kernels: bit-identical results): up to three views; the gather-side
   * prologue (in_scale / in_shift / in_relu) applied once per STAGED row, with one view; the training epilogues (TL_BF16, one view).
   * With in_all_ones the presence masks come from blk_pmask.  Other shapes fall through to `table` (TL_ERR_UNSUPPORTED without one). */
  const int32_t* blk_unit; const int32_t* blk_counter; const int32_t* blk_halo; const uint32_t* blk_lrb; const int32_t* blk_pmask;
  /* Scatter form of a one-hot table (table_one_hot = 1, K = 8: the inverse conv of reference blocks.py:113-123), i32[K][n_in]: the output
   * row that input row c feeds through tap k, or -1 -- i.e. the rulebook of the stride-2 conv whose pairs the inverse conv re-uses
   * (tl_level.child).  Optional (NULL: the gather forms run); when given, 16-bit launches of the widths of levels 1-4 walk the INPUT rows
   * instead: each read once, eight small products, rows scattered to the children that exist (csrc/tl_conv_up.hip).  Same results. */
  const int32_t* table_scatter;
  /* Optional split-bf16 copy of fp32 weights (tl_pack_weight_x3; TL_F32 launches only, NULL = absent).  When given, the kernel families
   * that serve the large levels (csrc/tl_conv_direct.hip, tl_conv_stream.hip) contract in the "bf16x3" form: every fp32 operand x is split in
   * registers into hi = bf16(x) and lo = bf16(x - hi), and a . b is formed as alo.bhi + ahi.blo + ahi.bhi on the bf16 matrix cores with fp32
   * accumulation -- storage, BatchNorm, residual and epilogues stay fp32, the contraction costs 3/16 of the fp32-input MFMA, products are
   * exact to ~2^-15 relative (the reference's fp32 inference, tree_learn/util/pipeline.py:86, within the 1e-3 parity gate at a third of
   * the exact mode's time).  Shapes without such an instantiation run the exact fp32 kernels on `weight`. */
  const void* weight_x3;
} tl_conv_args;

#define TL_EPI_NONE 0
#define TL_EPI_STATS 1
#define TL_EPI_BN_BWD 2
/* upper bound of the partial rows a tl_conv_fwd launch with epi_mode != 0 writes for n_out output rows */
int64_t tl_conv_red_parts(int64_t n_out);

int tl_conv_fwd(const tl_conv_args* args, tl_stream_t stream);
/* Which kernel(s) tl_conv_fwd would launch for `args`, without a GPU: runs the very same dispatch with every launch replaced by a record
 * "k_name<template args><<<grid, block, dynamic LDS bytes>>>" ("/f16" after the name: the float16 compilation of the kernel), records of a
 * conv that is two launches joined by " + ", written to buf (NUL-terminated, at most cap bytes).  Makes no HIP call and reads no memory
 * behind the pointers in `args` (any suitably aligned non-NULL value serves) except the host pointer red_nparts, which is written as by
 * tl_conv_fwd.  Returns what tl_conv_fwd would have returned (an empty route when that is an error), TL_ERR_ARG if the route did not fit.
 * Honours tl_set_tuning.  Per thread: another thread's tl_conv_fwd launches as usual meanwhile. */
int tl_conv_route(const tl_conv_args* args, char* buf, int cap);

/* Repack a reference-layout conv weight [Cout, k,k,k, Cin] (spconv `.weight`)
 * into the kernel layout [K=k^3][Cout][Cin] with dtype conversion. */
int tl_pack_weight(const float* w_ref, int Cout, int K, int Cin, void* w_packed, int dtype, tl_stream_t stream);
/* The split-bf16 form of a reference-layout fp32 conv weight for tl_conv_args.weight_x3 (Cin % 32 == 0): [K][Cout][Cin / 32][64 bf16] =
 * per 32-channel unit the hi parts bf16(w) of its four 8-channel MFMA pieces, then the lo parts bf16(w - hi): as many bytes as [K][Cout][Cin] fp32;
 * for Cin < 256 and Cout % 32 == 0 a second copy of the same bytes in MFMA-fragment order follows (1 KB contiguous per fragment load: the
 * small-level kernel).  tl_pack_weight_x3_bytes = the size of the buffer to pass. */
int64_t tl_pack_weight_x3_bytes(int Cout, int K, int Cin);
int tl_pack_weight_x3(const float* w_ref, int Cout, int K, int Cin, void* w_x3, tl_stream_t stream);
/* Weights of the input-gradient ("dgrad") conv of the same layer, for tl_conv_fwd over the transposed rulebook: w_t[k][ci][co] =
 * w_ref[co][flip ? K-1-k : k][ci] (taps flip for SubM convs: nbr[k][o] = i <=> nbr[K-1-k][i] = o), with dtype conversion. */
int tl_pack_weight_dgrad(const float* w_ref, int Cout, int K, int Cin, int flip, void* w_t, int dtype, tl_stream_t stream);
/* All three packings for many layers in ONE launch (a training step re-packs every conv weight after the optimizer: ~210 launches per
 * step otherwise).  descs (DEVICE array): src = the fp32 parameter [Cout][K][Cin], dst = the packed tensor in `dtype`, form 0 = tl_pack_weight,
 * 1 = tl_pack_weight_frag, 2 / 3 = tl_pack_weight_dgrad without / with flipped taps.  blocks (DEVICE, i32[n_blocks][2]): workgroup b writes
 * the 4096 output elements of descriptor blocks[b][0] starting at element 4096 * blocks[b][1]. */
typedef struct tl_pack_desc {
  const float* src;
  void* dst;
  int32_t Cout, K, Cin, form;
} tl_pack_desc;
int tl_pack_weights_batch(const tl_pack_desc* descs, const int32_t* blocks, int64_t n_blocks, int dtype, tl_stream_t stream);
/* Same weights in fragment order (Cout % 32 == 0, Cin % 32 == 0): [K][Cout/32][Cin/32][J][64 lanes][16 B], where lane
 * (fi = lane & 31, fh = lane >> 5) of 16-B piece j holds W[k][32 cb + fi][32 ch + (32 j + 16 fh) / sizeof(elem) ...]:
 * the B operand of one 32x32 MFMA step is one contiguous 1 KB block (J = 2 for bf16, 4 for fp32). */
int tl_pack_weight_frag(const float* w_ref, int Cout, int K, int Cin, void* w_frag, int dtype, tl_stream_t stream);

/* Weight gradient (training step; spconv's autograd behind the conv modules, tools/training/train.py:40):
 *   gw[k][co][ci] = sum_o gout[o][co] * x[table[k][o]][ci]   over the present rulebook entries, fp32.
 * x [n_in, x_ld >= Cin] and gout [n_out, g_ld >= Cout] in `dtype` (TL_F32, or TL_BF16 = mixed-precision training: widened
 * to fp32 in registers; TL_F16 likewise), table i32[K][n_out] or NULL (K = 1: identity), gw f32[K][Cout][Cin] out (fully written),
 * ws f32[tl_conv_wgrad_ws_floats(...)] scratch.  Deterministic. */
int64_t tl_conv_wgrad_ws_floats(int64_t n_out, int K, int Cin, int Cout);
int tl_conv_wgrad(const void* x, int64_t x_ld, const void* gout, int64_t g_ld, int dtype, const int32_t* table, int64_t n_out,
                  int64_t n_in, int K, int Cin, int Cout, float* gw, float* ws, tl_stream_t stream);
/* the same with gw written in the reference parameter layout f32[Cout][K][Cin] (= spconv `.weight` [Cout,k,k,k,Cin]: the `.grad` of the
 * module parameter, no transposing copy afterwards); Cin % 4 == 0 */
int tl_conv_wgrad_ref(const void* x, int64_t x_ld, const void* gout, int64_t g_ld, int dtype, const int32_t* table, int64_t n_out,
                      int64_t n_in, int K, int Cin, int Cout, float* gw, float* ws, tl_stream_t stream);

/* The weight gradient of a 27-tap 32 -> 32 SubM conv over a BLOCK-LOCAL level (tl_blk_build: x and gout rows in the new order) in the
 * staged-unit form of the forward kernel: a unit's own and halo rows of x, its gout rows and its local rulebook are staged in LDS once and all
 * 27 taps contract against them, instead of 27 gathers per output row through the plain table (level 1 of the training step,
 * tools/training/train.py:40).  16-bit dtypes, Cin = Cout = 32; anything else returns TL_ERR_UNSUPPORTED and the caller uses tl_conv_wgrad over
 * tl_blk.nn.  gw f32[27][32][32], or f32[32][27][32] with ref_layout != 0; ws f32[tl_conv_wgrad_blk_ws_floats()].  Deterministic. */
int64_t tl_conv_wgrad_blk_ws_floats(void);
int tl_conv_wgrad_blk(const void* x, int64_t x_ld, const void* gout, int64_t g_ld, int dtype, const int32_t* blk_unit, const int32_t* blk_counter,
                      const int32_t* blk_halo, const uint32_t* blk_lrb, int64_t n, int Cin, int Cout, float* gw, int ref_layout, float* ws,
                      tl_stream_t stream);

/* ------------------------------------------------------------------ per-point heads
 * Replaces forward_head (tree_learn.py:97-103): features[v2p] gather, output_layer BN+ReLU
 * (tree_learn.py:42,93) as prologue, then both MLPs (blocks.py:8-18) with eval-mode BN folded:
 *   h = relu(W1' f + b1'),  y = W2 h + b2.
 * feats [M,C] (dtype), v2p i64[N]; w1 f32[2][C][C], b1 f32[2][C] (BN folded), w2 f32[5][C] (2 semantic rows
 * then 3 offset rows), b2 f32[5].  backbone f32[N,C] may be NULL (skip the 128 B/point write). */
int tl_head_mlp(const void* feats, int64_t feats_ld, int dtype, int C, const int64_t* v2p, int64_t N,
                const float* pro_scale, const float* pro_shift,
                const float* w1, const float* b1, const float* w2, const float* b2,
                float* backbone, float* logits, float* offsets, tl_stream_t stream);

/* ------------------------------------------------------------------ elementwise helpers */
/* out = relu?(in * scale + shift) over [n, C] with row strides (BatchNorm1d eval + ReLU, tree_learn.py:42). */
int tl_affine_relu(const void* in, int64_t in_ld, void* out, int64_t out_ld, int64_t n, int C, int dtype,
                   const float* scale, const float* shift, int relu, tl_stream_t stream);

/* ------------------------------------------------------------------ BatchNorm1d, training mode (+ ReLU)
 * The `norm_fn(C), nn.ReLU()` pair in front of every conv and inside both heads in TRAINING mode (reference
 * tree_learn/model/blocks.py:55-70,102-123, tree_learn.py:34-46: BatchNorm1d(eps=1e-4, momentum=0.1) over all active voxels of
 * the batch; exercised by tools/training/train.py:30-44).  Replaces ATen's batch_norm / relu forward and backward kernels.
 * Deterministic (fixed row partition, fp64 partial sums added in a fixed order, no atomics).
 *
 * tl_bn_train_stats: x [n, C] (f32 or bf16, row stride ld) -> mean, rstd = 1/sqrt(var_biased + eps), scale = gamma * rstd,
 *   shift = beta - mean * scale (all f32[C]); running_mean / running_var (nullable pair) get the momentum update with the
 *   UNBIASED variance like torch, num_batches_tracked (nullable, i64[1]) += 1.  y = relu(x * scale + shift) is then one
 *   tl_affine_relu call.  ws f64[tl_bn_ws_doubles(n, C)].  C % 4 == 0, C <= 1024.
 * tl_bn_train_bwd: dy [n, C] (f32 or bf16) = gradient w.r.t. y -> dx [n, C] in x's dtype, dgamma, dbeta f32[C]; `relu` != 0
 *   masks dy where y <= 0 (y is recomputed from x); dx_add (nullable, x's dtype, [n, C]) is added to dx in the same pass -- the
 *   gradient reaching x along its OTHER use (the residual / skip connection: x feeds both this BatchNorm and an identity path), so
 *   autograd's separate accumulation kernel disappears.  Under mixed precision (the reference trains under autocast,
 *   tools/training/train.py:32) activations and their gradients stay bf16 between layers; all statistics are fp64 / fp32. */
int64_t tl_bn_ws_doubles(int64_t n, int C);
int tl_bn_train_stats(const void* x, int64_t ld, int64_t n, int C, int dtype, const float* gamma, const float* beta, float eps,
                      float momentum, double* ws, float* mean, float* rstd, float* scale, float* shift, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, tl_stream_t stream);
int tl_bn_train_bwd(const void* x, int64_t ld, int x_dtype, const void* dy, int64_t dld, int dy_dtype, int64_t n, int C,
                    const float* mean, const float* rstd, const float* scale, const float* shift, int relu, double* ws,
                    float* dgamma, float* dbeta, void* dx, int64_t xld, const void* dx_add, int64_t dx_add_ld, tl_stream_t stream);

/* The same BatchNorm with its reductions taken from a conv epilogue (tl_conv_args.epi_mode): part f64[nparts][2][C] as written by
 * tl_conv_fwd.  tl_bn_train_finish = the second half of tl_bn_train_stats (partial sums of x and x^2 -> mean .. shift, running
 * statistics); tl_bn_train_bwd_from_parts = the second half of tl_bn_train_bwd for an ALREADY masked g (TL_EPI_BN_BWD: sums of g and
 * g * xhat -> dgamma, dbeta, then dx = scale * (g - dbeta / n - xhat * dgamma / n) + dx_add in one pass over x and g; C % 8 == 0 and
 * 16-B aligned rows, else TL_ERR_UNSUPPORTED). */
int tl_bn_train_finish(const double* part, int64_t nparts, int64_t n, int C, const float* gamma, const float* beta, float eps, float momentum, float* mean,
                       float* rstd, float* scale, float* shift, float* running_mean, float* running_var, int64_t* num_batches_tracked, tl_stream_t stream);
int tl_bn_train_bwd_from_parts(const void* x, int64_t ld, int x_dtype, const void* g, int64_t gld, int g_dtype, int64_t n, int C, const float* mean,
                               const float* rstd, const float* scale, const float* shift, const double* part, int64_t nparts, float* dgamma, float* dbeta,
                               void* dx, int64_t xld, const void* dx_add, int64_t dx_add_ld, tl_stream_t stream);

/* out f32[n, Cout] = x[n, Cin] . W^T for Cout <= 8 (the output Linears of the two heads in training, blocks.py:8-26 `MLP`): x and W
 * [Cout][Cin] in `dtype`, fp32 accumulation AND fp32 result -- under mixed precision the logits / offsets keep fp32 resolution. */
int tl_linear_small_f32(const void* x, int64_t x_ld, int dtype, const void* w, int Cin, int Cout, int64_t n, float* out, int64_t out_ld,
                        tl_stream_t stream);

/* Voxel -> point feature gather and its gradient (tree_learn.py:98 `output.features[v2p_map]`; tools/training/train.py:40):
 *   tl_gather_rows     : out[p, :] = in[idx[p], :] for p < N (idx < 0 counts from the end like torch indexing; in [n_rows, C]);
 *   tl_scatter_add_rows: gin[v, :] = sum over the points p with idx[p] == v of g[p, :], added in ascending p in fp32; `order` i64[N] =
 *                        the STABLE argsort of idx, sorted_idx = idx[order], idx NORMALISED to 0 <= idx < n_rows before the sort
 *                        (points are grouped by equal sorted values: -1 and n_rows - 1 would be two groups writing one row); gin
 *                        [n_rows, C] contiguous, fully written (rows without a point are zero).  Deterministic, no atomics.  C * sizeof(elem) % 16 == 0, 16-B aligned rows. */
int tl_gather_rows(const void* in, int64_t in_ld, int dtype, int C, int64_t n_rows, const int64_t* idx, int64_t N, void* out, int64_t out_ld, tl_stream_t stream);
int tl_scatter_add_rows(const void* g, int64_t g_ld, int dtype, int C, const int64_t* order, const int64_t* sorted_idx, int64_t N, int64_t n_rows, void* gin,
                        int64_t gin_ld, tl_stream_t stream);

/* Keep rows where mask != 0 (masks_inner filtering before D2H, util/pipeline.py:100-103).
 * in f32[n,C] -> out f32[count,C]; count i32[1] device.  Stable (input order kept).
 * ws i32[tl_compact_ws_words(n)] scratch. */
int64_t tl_compact_ws_words(int64_t n);
int tl_compact_rows(const float* in, int C, const uint8_t* mask, int64_t n, float* out, int32_t* count,
                    int32_t* ws, tl_stream_t stream);

/* ------------------------------------------------------------------ inference tiling
 * Replaces, per tile, the box masks + `.cpu()` + np.savez / np.load round trip of
 * SampleGenerator.tile_generate_and_save (tree_learn/util/data_preparation.py:393-441,456-476) and the
 * bookkeeping of TreeDataset.__getitem__ (tree_learn/dataset/dataset.py:34-76,87-91), plot arrays resident in HBM.
 *   xyz f32[n,3], label f32[n], feat f32[n,F] : the voxelised plot;
 *   box (HOST struct): outer = (xmin,xmax,ymin,ymax) as float32 (closed box, compared in float32),
 *       inner = the inner square in float64 (x in [x0,x1), y in (y0,y1], compared in float64),
 *       center = tile centre subtracted in float64, half_inner = inner_square_edge_length / 2;
 *   outputs, capacity n rows, rows kept in plot order: coords f32[.,3] (centred), out_feat f32[.,F],
 *   instance_labels i64 (int32 truncation of label), semantic_labels i64 (label 0 -> 1, else 0),
 *   mask_inner u8, mask_sem u8 (= inner & label != -1);
 *   count i32[2] device out = {rows kept, rows inside the inner square};  ws i32[tl_tile_crop_ws_words(n)]. */
typedef struct tl_tile_box {
  float outer[4];
  double inner[4];
  double center[2];
  float half_inner;
} tl_tile_box;
int64_t tl_tile_crop_ws_words(int64_t n);
int tl_tile_crop(const float* xyz, const float* label, const float* feat, int64_t n, int F, const tl_tile_box* box,
                 float* coords, float* out_feat, int64_t* instance_labels, int64_t* semantic_labels,
                 uint8_t* mask_inner, uint8_t* mask_sem, int32_t* count, int32_t* ws, tl_stream_t stream);

/* ------------------------------------------------------------------ plot preparation
 * Global voxel down-sample and verticality feature, delegated by the reference to open3d 0.17.0
 * (VoxelDownSampleAndTrace; tree_learn/util/data_preparation.py:60-79) and jakteristics 0.5.1
 * (compute_features, data_preparation.py:82-88; called from generate_tiles, util/pipeline.py:40-65).
 *
 * tl_cell_keys: key[i] = pack(floor((p - min_bound) / cell) - base3), 21 bits per axis, z in the low bits;
 *   round_input != 0 rounds the coordinates to 2 decimals first (np.round(points, 2), data_preparation.py:62);
 *   base3 = HOST i64[3]; err i32[1] device out is set when a cell index leaves the 21-bit range.
 * tl_downsample_reduce: keys sorted ascending with the stable permutation `perm` (host code: torch.sort);
 *   per voxel, in input order and in double: mean of the 2-decimal-rounded points -> float32 -> rounded to 2
 *   decimals (util/pipeline.py:44-45); first_idx = smallest original index of the voxel (`idx_keep`);
 *   point2vox i64[n] = voxel row of every original point (the trace); n_voxels i64[1] device out.
 * tl_verticality: xyz_sorted f64[n,3] and keys sorted by a `radius`-sized cell key (tl_cell_keys, round_input = 0);
 *   extent2 = HOST i64[2] largest cell index in x and y; out f32[n] (sorted order) = 1 - |n_z| of the sample
 *   covariance of all points within `radius` (inclusive, the point itself included); NaN when fewer than 3. */
int tl_cell_keys(const double* xyz, int64_t n, double cell, double min_bound, const int64_t* base3, int round_input,
                 int64_t* keys, int32_t* err, tl_stream_t stream);
int64_t tl_downsample_ws_words(int64_t n);
int tl_downsample_reduce(const double* xyz, const int64_t* sorted_keys, const int64_t* perm, int64_t n, float* out_xyz,
                         int64_t* first_idx, int64_t* point2vox, int64_t* n_voxels, int32_t* ws, tl_stream_t stream);
/* tl_downsample_reduce_r64: the same, but the double mean is rounded to 2 decimals in double and then cast to float32, the
 *   order of the training-data generator (np.round(data, 2).astype(np.float32), tools/data_gen/gen_train_data.py:40-42). */
int tl_downsample_reduce_r64(const double* xyz, const int64_t* sorted_keys, const int64_t* perm, int64_t n, float* out_xyz,
                             int64_t* first_idx, int64_t* point2vox, int64_t* n_voxels, int32_t* ws, tl_stream_t stream);
/* Group means for `ensemble` (tree_learn/util/pipeline.py:113-141: pandas groupby(['x','y','z']).mean() over the rounded
 * coordinates): keys sorted ascending with the stable permutation `perm`; per group and column the double-precision sum of
 * the members in input order divided by their number.  src f32[n,C]; mean f64[n,C] capacity (first n_groups rows written);
 * first_idx i64 = smallest original index of each group; ws i32[tl_downsample_ws_words(n)].  Deterministic. */
int tl_group_mean(const float* src, int64_t n, int C, const int64_t* sorted_keys, const int64_t* perm, double* mean,
                  int64_t* first_idx, int64_t* n_groups, int32_t* ws, tl_stream_t stream);
int tl_verticality(const double* xyz_sorted, const int64_t* sorted_keys, int64_t n, double radius, const int64_t* extent2,
                   float* out, tl_stream_t stream);

/* ------------------------------------------------------------------ geometric point features
 * Replaces jakteristics.compute_features(points, search_radius, feature_names=[...]) for ANY list of its feature
 * names (data_preparation.py:82-88, "verticality (and optionally other features)").  jakteristics is not part of
 * the reference tree: the definitions are restated (parity unpinned, as for tl_verticality).
 *
 * tl_eigen_features: xyz_sorted f64[n,3], sorted_keys and extent2 as for tl_verticality (tl_cell_keys with a
 *   `radius`-sized cell, round_input = 0, sorted with z fastest).  piece_start i64[n_pieces] device: the work table,
 *   ascending or not: the sorted index of every point that starts an (x, y) column of cells (key >> 21 differs from
 *   its predecessor's) or whose index is a multiple of 64; one wave serves one piece, the points from there to the
 *   next such index.  A point whose piece is missing from the table is not written.  cols = HOST i32[F] feature ids,
 *   1 <= F <= TL_FEAT_COUNT;
 *   out f32[n,F] in sorted order.  Neighbourhood: squared distance <= radius^2, the point itself included; sums of
 *   d and d d^T relative to the query point in f64, added in the order of the sorted array; sample covariance
 *   (n - 1); all eigenpairs by cyclic Jacobi in f64 with l1 >= l2 >= l3 clamped at 0 and every eigenvector oriented
 *   by z >= 0 (z == 0: y >= 0; that 0 too: x >= 0).  Fewer than 3 neighbours: NaN in every column except
 *   number_of_neighbors; a ratio with a zero denominator is NaN.  Ids, with s = l1 + l2 + l3:
 *    0 eigenvalue_sum s          1 omnivariance cbrt(l1 l2 l3)   2 eigenentropy -sum l ln l (0 ln 0 = 0)
 *    3 anisotropy (l1-l3)/l1     4 planarity (l2-l3)/l1          5 linearity (l1-l2)/l1
 *    6 PCA1 l1/s                 7 PCA2 l2/s                     8 surface_variation l3/s
 *    9 sphericity l3/l1         10 verticality 1-|e3z|          11..13 nx ny nz = e3
 *   14 number_of_neighbors      15..17 eigenvalue1..3           18..26 eigenvector1x .. eigenvector3z
 *   Compiled without contraction: the same bits on every run, whatever the piece table's order.  One launch, no
 *   atomics.  TL_ERR_ARG on a null pointer, n or n_pieces <= 0, n_pieces > n, F or an id out of range. */
enum { TL_FEAT_COUNT = 27 };
int tl_eigen_features(const double* xyz_sorted, const int64_t* sorted_keys, int64_t n, double radius, const int64_t* extent2,
                      const int64_t* piece_start, int64_t n_pieces, const int32_t* cols, int F, float* out, tl_stream_t stream);
/* tl_eigen_features_scales: the same features at S radii in one launch and one walk over the candidates.  The arrays are
 *   those of tl_eigen_features with cells of the LARGEST radius, radii[S - 1].  radii = HOST f64[S], finite, > 0, strictly ascending,
 *   1 <= S <= TL_FEAT_MAX_SCALES.  out f32[n, S, F] in sorted order: out[i, k, :] is, bit for bit, the row i that tl_eigen_features
 *   writes on the same sorted arrays with radius = radii[k] (every scale has its own count and sums, taken over the candidates with
 *   squared distance <= radii[k]^2 in the order of the sorted array).  No atomics, no scratch.  TL_ERR_ARG, nothing launched: whatever
 *   tl_eigen_features refuses, S out of range, a radius that is NaN, infinite, <= 0 or not above its predecessor. */
#define TL_FEAT_MAX_SCALES 4
int tl_eigen_features_scales(const double* xyz_sorted, const int64_t* sorted_keys, int64_t n, const double* radii, int S, const int64_t* extent2,
                             const int64_t* piece_start, int64_t n_pieces, const int32_t* cols, int F, float* out, tl_stream_t stream);

/* ------------------------------------------------------------------ random training crops
 * The random-crop half of SampleGenerator (tree_learn/util/data_preparation.py:136-330) on a plot resident in HBM; the
 * grid and candidate lay-out stay on the host (util/crops.py).  f64 wherever the reference is f64, no fma contraction.
 *
 * tl_crops_occupancy <- get_occupancy_grid (data_preparation.py:154-166): xy f32[n,2] = the subsampled valid points;
 *   x_steps f64[x_dim+1], y_steps f64[y_dim+1] ascending; grid u8[x_dim,y_dim] out = 1 where some point has
 *   steps[i] < x <= steps[i+1] in x and in y (lower-bound search, exact f64 compare of the widened f32).
 * tl_crops_fill <- fill_holes (data_preparation.py:571-586): an empty cell of `raw` becomes 1 when the occupied cells of the
 *   window of +-how_far_fill cells, clipped at the borders, make count / (h*w) >= min_percent_occupied_fill (f64);
 *   occupied cells stay 1.  filled u8[x_dim,y_dim] out, distinct from raw.
 * tl_crops_check <- check_occupancy (data_preparation.py:209-230): one workgroup per candidate; cell (i, j) has the centre
 *   (cell_x[i], cell_y[j]) f64 and is kept when max(|u|, |v|) <= chunk_size / 2 for (u, v) = (c - centre) @ Rinv.T, the
 *   centre f32[k,2] widened, rinv f64[k,2,2] row-major.  sums f64[k] = sum of the kept cells' occupancy; pass u8[k] =
 *   sums / denominator > min_percent_occupied_choose.  Either output may be null, not both.
 * tl_crops_count / tl_crops_extract <- save (data_preparation.py:264-289), for a batch of 1..32 crops per plot read:
 *   xyz f32[n,3], label f32[n], feat f32[n,F] the plot; a row belongs to crop c when max(|u|, |v|) <= chunk_size / 2 for
 *   (u, v) = f64(xy - centre_c, a float32 subtraction) @ Rinv_c.T.  tl_crops_count writes counts i32[n_crops] (device) and
 *   the row offsets into ws i32[tl_crops_ws_words(n, n_crops)]; tl_crops_extract then writes the crops one after another,
 *   each in plot row order: out_xyz f32[.,3] = (f32 u, f32 v, z), out_label i32 (truncated label), out_feat f32[.,F];
 *   rows at or beyond `capacity` are not written.  Offsets are int32: n * n_crops must stay below 2^31 (else TL_ERR_ARG). */
int tl_crops_occupancy(const float* xy, int64_t n, const double* x_steps, int x_dim, const double* y_steps, int y_dim, uint8_t* grid,
                       tl_stream_t stream);
int tl_crops_fill(const uint8_t* raw, int x_dim, int y_dim, int how_far_fill, double min_percent_occupied_fill, uint8_t* filled,
                  tl_stream_t stream);
int tl_crops_check(const double* cell_x, int x_dim, const double* cell_y, int y_dim, const uint8_t* occupancy, const float* centres,
                   const double* rinv, int64_t n_candidates, double chunk_size, double denominator, double min_percent_occupied_choose,
                   double* sums, uint8_t* pass, tl_stream_t stream);
int64_t tl_crops_ws_words(int64_t n, int n_crops);
int tl_crops_count(const float* xyz, int64_t n, int n_crops, const float* centres, const double* rinv, double chunk_size, int32_t* counts,
                   int32_t* ws, tl_stream_t stream);
int tl_crops_extract(const float* xyz, const float* label, const float* feat, int64_t n, int F, int n_crops, const float* centres,
                     const double* rinv, double chunk_size, const int32_t* ws, int64_t capacity, float* out_xyz, int32_t* out_label,
                     float* out_feat, tl_stream_t stream);

/* ------------------------------------------------------------------ outlier removal on crops and tiles (csrc/tl_outlier.hip)
 * sor_filter / rad_filter (tree_learn/util/data_preparation.py:589-614): open3d's remove_statistical_outlier and
 * remove_radius_outlier, which SampleGenerator applies to every training crop (:281-287) and every tile (:446-454).  open3d is not
 * part of the reference tree; the semantics below are the specification (restated from open3d 0.17 / nanoflann, parity unpinned).
 * All arithmetic is f64 without fma contraction: d2(i, j) = (dx*dx + dy*dy) + dz*dz, d = sqrt(d2) correctly rounded.
 *
 * Grid: cell = floor((p - lo) / h) per axis, dims[a] cells (1 .. 2^21) along axis a; key = the three cell indices bit-interleaved
 *   (Morton order, x highest).  The caller sorts the keys (keys_sorted) and gathers the points in that order (xyz_sorted f64[n,3]);
 *   perm i64[n] = original row of sorted row.  Outputs are written in ORIGINAL row order.  Any h > 0 gives the same results.
 * tl_outlier_keys: keys i64[n]; *err (device) = 1 when a point falls outside the grid (its key is then 0), else 0.
 *   dims outside 1 .. 2^21 or h <= 0: TL_ERR_UNSUPPORTED (the caller grows the cell).
 * tl_knn_mean_dist: avg[i] = (sum of the min(k, n) smallest d(i, .), point i itself included at 0, added in ascending order one
 *   after the other) / min(k, n).  Bit-identical for any grid, launch geometry and row order.  k in 1..64, else TL_ERR_UNSUPPORTED.
 * tl_sor_keep: mean = (sum of avg[i] over avg[i] > 0) / n; std = sqrt((sum of (avg[i] - mean)^2 over avg[i] > 0) / (n - 1));
 *   *thr (device) = mean + std_ratio * std; keep[i] = avg[i] > 0 && avg[i] < thr.  n = 1 keeps nothing (*thr = 0).  Both sums are
 *   fixed trees over fixed 2048-row chunks: no float atomics, the same bits run to run and for any grid size.
 *   ws f64[tl_sor_ws_doubles(n)].
 * tl_radius_count: count[i] = number of j, i included, with d2(i, j) < radius * radius (strict).  Needs h >= 1.0001 * radius
 *   (else TL_ERR_ARG): the ball then lies inside the 27 cells around the point's own. */
int tl_outlier_keys(const double* xyz, int64_t n, const double lo[3], double h, const int32_t dims[3], int64_t* keys, int32_t* err,
                    tl_stream_t stream);
int tl_knn_mean_dist(const double* xyz_sorted, const int64_t* keys_sorted, const int64_t* perm, int64_t n, const double lo[3], double h,
                     const int32_t dims[3], int k, double* avg, tl_stream_t stream);
int64_t tl_sor_ws_doubles(int64_t n);
int tl_sor_keep(const double* avg, int64_t n, double std_ratio, uint8_t* keep, double* thr, double* ws, tl_stream_t stream);
int tl_radius_count(const double* xyz_sorted, const int64_t* keys_sorted, const int64_t* perm, int64_t n, const double lo[3], double h,
                    const int32_t dims[3], double radius, int32_t* count, tl_stream_t stream);

/* ------------------------------------------------------------------ two epochs of one plot (csrc/tl_change.hip)
 * The hot path of rigid registration (ICP), cloud-to-cloud distances and tree matching between two scans.  The semantics are the
 * project's own; tests/change_restatement.py states them in numpy and is the specification.  All arithmetic is f64 without fma
 * contraction, every operation rounded on its own; f32 queries are widened first.
 *
 * Queries: q = f32 (dtype_f64 = 0) or f64 (dtype_f64 = 1) [nq, >= 3] with a row stride of ld elements (ld >= 3), in their original
 *   order.  T = HOST pointer to 12 doubles, a row-major 3 x 4 rigid transform handed to the kernel by value; NULL = identity.
 *   moved query  x'_a = ((T[a][0]*x + T[a][1]*y) + T[a][2]*z) + T[a][3]  per axis a.
 * Reference: binned and sorted exactly as for the outlier section above (tl_outlier_keys, one sort): xyz_sorted f64[nr,3],
 *   keys_sorted, perm i64[nr] = original row of sorted row, and the grid lo, h, dims.
 *
 * tl_cross_nn: nn i64[nq], d2 f64[nq]: over the reference rows j with d2(i, j) = (dx*dx + dy*dy) + dz*dz < max_dist * max_dist
 *   (strict) the smallest d2 and the ORIGINAL row that has it; among equal d2 the smaller original row.  No such row, or a moved
 *   query that is not finite: nn = -1, d2 = +inf.  The moved query may lie anywhere (its cell index is clamped in f64; up to one cell
 *   outside the grid it still sees the border cells).  Needs h >= 1.0001 * max_dist (else TL_ERR_ARG): the ball then lies inside the
 *   27 cells around the query's own.  nr = 0 writes -1 / +inf for every query (the reference pointers and the grid are not looked
 *   at); nq = 0 returns TL_OK without a launch.  The results do not depend on the grid, the launch or the reference's row order.
 * tl_rigid_sums: sums f64[17] (device) of one ICP step over the rows i with 0 <= nn[i] < nr and d2[i] < reject2.  ref f64[nr,3] is
 *   the reference in ORIGINAL row order, c[3] (host) a centre that keeps the products small.  With a = x'_i - c and b = ref[nn[i]] - c
 *   a row contributes 1.0, a (3), b (3), the outer product a b^T row-major (9, each a single multiply) and d2[i]; any other row
 *   contributes +0.0 to all 17.  Every sum is a fixed tree: rows in chunks of 2048 in row order, within a chunk
 *   s[i] += s[i + stride] for stride 1024 .. 1 with missing rows at +0.0, then the same tree over the chunk partials, 2048 at a
 *   time, until one is left.  No atomics: the same bits on every run and for any launch geometry.  nq = 0 gives 17 zeros.
 *   ws f64[tl_rigid_sums_ws_doubles(nq)].
 * Null or misaligned pointers and bad sizes are refused (TL_ERR_ARG) before anything else. */
int tl_cross_nn(const double* xyz_sorted, const int64_t* keys_sorted, const int64_t* perm, int64_t nr, const double lo[3], double h,
                const int32_t dims[3], const void* q, int dtype_f64, int64_t ld, int64_t nq, const double* T, double max_dist, int64_t* nn,
                double* d2, tl_stream_t stream);
int64_t tl_rigid_sums_ws_doubles(int64_t nq);
int tl_rigid_sums(const void* q, int dtype_f64, int64_t ld, int64_t nq, const double* T, const int64_t* nn, const double* d2, const double* ref,
                  int64_t nr, const double c[3], double reject2, double* sums, double* ws, tl_stream_t stream);

/* ------------------------------------------------------------------ clustering
 * Replaces sklearn DBSCAN(eps, min_samples=2) in group_dbscan (tree_learn/util/pipeline.py:173-180):
 * connected components of the eps-graph on 2-D points; isolated points = -1; component labels
 * 0..K-1 ordered by the smallest point index of each component (sklearn's numbering).
 * xy f32[n,2]; labels i32[n] out; n_clusters i32[1] device out;
 * ws: tl_cluster_ws_bytes(n) bytes. */
int64_t tl_cluster_ws_bytes(int64_t n);
int tl_cluster_grid(const float* xy, int64_t n, double eps, int32_t* labels, int32_t* n_clusters,
                    void* ws, tl_stream_t stream);

/* HDBSCAN(min_cluster_size = m) of group_hdbscan (tree_learn/util/pipeline.py:184-191; sklearn: min_samples = m,
 * euclidean, Prim MST on mutual reachability, EOM).  Device stage: core distances (k-th neighbour incl. self) and
 * Prim's MST with sklearn's tie-breaking, fp64 on the fp32 points.  xy f32[n,2]; e_src/e_dst i32[n-1], e_w f64[n-1]
 * (edges in insertion order); core f64[n] or NULL; ws tl_hdbscan_ws_bytes(n). */
int64_t tl_hdbscan_ws_bytes(int64_t n);
int tl_hdbscan_mst(const float* xy, int64_t n, int min_samples, int32_t* e_src, int32_t* e_dst, double* e_w,
                   double* core, void* ws, tl_stream_t stream);
/* HOST stage (host pointers, no GPU work): edges -> single linkage -> condensed tree -> EOM -> labels i32[n]
 * (-1 noise, clusters numbered by ascending condensed-tree id like sklearn). */
int tl_hdbscan_labels_host(const int32_t* e_src, const int32_t* e_dst, const double* e_w, int64_t n,
                           int min_cluster_size, int32_t* labels);

/* The same device stage for large inputs (csrc/tl_hdbscan_grid.hip): core distances and the mutual-reachability MST through a
 * quadtree over a uniform cell grid -- grid k-NN for the core distances, Boruvka rounds for the tree -- instead of two O(n^2)
 * passes.  Same arithmetic (fp64 on the fp32 points), so core distances are bit-identical to tl_hdbscan_mst and the MST has the
 * same weight multiset; among equal-weight edges it takes the one that is smallest under (weight, smaller index, larger index)
 * instead of Prim's insertion order, and it returns the edges unordered (e_src < e_dst; pass them through
 * tl_hdbscan_prim_order_host before tl_hdbscan_labels_host).
 *   tl_hdbscan_grid_plan: picks the grid (bounding box; leaf level such that an occupied cell holds about eight points); ws of
 *     tl_hdbscan_grid_plan_ws_bytes(); SYNCHRONISES the stream (two small read-backs).
 *   tl_hdbscan_mst_grid: ws of tl_hdbscan_grid_ws_bytes(n, grid); SYNCHRONISES the stream once per Boruvka round (<= ~20).
 *     min_samples up to 4096 (reference util/pipeline.py:184-191 passes any tau_min): beyond 128 the k-best lists are heaps in the
 *     workspace -- size it with tl_hdbscan_grid_ws_bytes_k(n, grid, min_samples). */
typedef struct TlHdbGrid {
  double lo[2];     /* lower corner of the bounding box */
  double h;         /* leaf cell edge */
  int32_t levels;   /* leaf grid = 2^levels x 2^levels cells, 0..13 */
  int32_t reserved;
} TlHdbGrid;
int64_t tl_hdbscan_grid_plan_ws_bytes(void);
int tl_hdbscan_grid_plan(const float* xy, int64_t n, TlHdbGrid* grid, void* ws, tl_stream_t stream);
int64_t tl_hdbscan_grid_ws_bytes(int64_t n, const TlHdbGrid* grid);
int64_t tl_hdbscan_grid_ws_bytes_k(int64_t n, const TlHdbGrid* grid, int min_samples);
int tl_hdbscan_mst_grid(const float* xy, int64_t n, int min_samples, const TlHdbGrid* grid, int32_t* e_src, int32_t* e_dst,
                        double* e_w, double* core, void* ws, tl_stream_t stream);
/* HOST stage: spanning-tree edges in any order / orientation -> the order and orientation Prim's algorithm started at point 0
 * gives them (lightest frontier edge, smallest new index among equal weights, src = the end already in the tree), which is what
 * tl_hdbscan_labels_host's tie-breaking and cluster numbering key on.  All arrays i32/f64[n-1], host memory. */
int tl_hdbscan_prim_order_host(const int32_t* e_src, const int32_t* e_dst, const double* e_w, int64_t n, int32_t* o_src,
                               int32_t* o_dst, double* o_w);

/* ------------------------------------------------------------------ next-row helpers
 * k-NN majority vote: replaces KNeighborsClassifier(n_neighbors=k).fit(ref, labels).predict(query) in
 * assign_remaining_points_nearest_neighbor (tree_learn/util/pipeline.py:287-296).  ref_xyz f32[nr,3], ref_label i64[nr],
 * q_xyz f32[nq,3] -> out_label i64[nq]; k in {1,3,5}; ties -> smallest label; fp64 distances. */
int tl_knn_vote(const float* ref_xyz, const int64_t* ref_label, int64_t nr, const float* q_xyz, int64_t nq, int k,
                int64_t* out_label, tl_stream_t stream);
/* The same vote over a uniform cell grid (exact; bit-identical to tl_knn_vote): the caller bins the reference points
 * (cell = floor(((double)p - (double)lo) * (double)(1.0f / h)) per axis, each operation rounded on its own,
 * key = (cx * dims[1] + cy) * dims[2] + cz), sorts them by key and passes the
 * sorted coordinates / labels / ORIGINAL indices, the ncells distinct keys ascending and their row ranges cell_start[ncells + 1].
 * 1 <= dims[a] <= 2^20 per axis, else TL_ERR_ARG: the ring bound is argued for fp64 binning over at most 2^20 cells (fp32 binning
 * moved cell borders by more than the bound's 0.1 % margin from about 2 * 10^4 cells per axis on).
 * A query walks Chebyshev rings of cells until its k-th best distance beats anything an unvisited ring can hold; ties are broken
 * by (distance, original index) as in the brute-force form.  O(nq * points near the query) instead of O(nq * nr). */
int tl_knn_vote_grid(const float* ref_sorted_xyz, const int64_t* ref_sorted_label, const int64_t* ref_sorted_index, int64_t nr,
                     const int64_t* cell_keys, const int64_t* cell_start, int64_t ncells, const float lo[3], float h, const int32_t dims[3],
                     const float* q_xyz, int64_t nq, int k, int64_t* out_label, tl_stream_t stream);

/* ------------------------------------------------------------------ scoring a segmentation against ground truth (csrc/tl_eval.hip)
 * Contingency table: replaces the P x G masked loop of get_detections (tree_learn/util/eval.py:7-25) and the per-pair masks of
 * evaluate_no_partition (:100-123).  pred, gt i64[n] (n < 2^31) -> table i64[(n_pred + 1) * (n_gt + 1)] (overwritten), row-major:
 * row 0 = every negative pred, row p + 1 = pred p (p < n_pred); column 0 = gt == non_tree_label or gt < 0, column g + 1 = gt g
 * (g < n_gt).  Points outside those ranges are not counted.  Exact integer counts (deterministic); every detection matrix follows
 * from the table on the host in fp64 (tp = C, fp = row sum - C, fn = column sum - C). */
int tl_eval_contingency(const int64_t* pred, const int64_t* gt, int64_t n, int64_t n_pred, int64_t n_gt, int64_t non_tree_label,
                        int64_t* table, tl_stream_t stream);
/* Radial / vertical bands of matched trees: replaces evaluate_xy_partition (eval.py:127-178) and evaluate_z_partition (:182-226).
 *   xyz f64[n,3]; gt, pred i64[n]; gt_order i64[n] with gt_start i64[n_gt + 1]: the points of gt tree g are
 *   gt_order[gt_start[g] .. gt_start[g+1]) in ascending point order (a stable sort); pred_order / pred_start likewise for n_pred
 *   predictions; pairs i64[m,2] = (gt g, pred p); edges f64[n_edges] (2 <= n_edges <= 257).
 *   Out: tp, fp, fn i64[m, n_edges - 1] -- band k holds the points whose value v satisfies v >= edges[k] && v < edges[k+1]; a point of
 *   gt g is tp if its pred is p, fn otherwise; a point of pred p whose gt is not g is fp -- and norm f64[m,3]:
 *   TL_EVAL_XY: (position x, position y, regularised max), v = |xy - position| / regularised max, position = mean xy of the tree points
 *     with z <= min z + 0.30 (summed in point order, eval.py:147-151), regularised max = 5th-largest v numerator over the tree (:156-160);
 *   TL_EVAL_Z: (min z, regularised max, 0), v = (z - min z) / (regularised max - min z), regularised max = 5th-largest z (:203-208).
 *   All value arithmetic in fp64 in the reference's operation order, no fma contraction.  One workgroup per pair; the caller ensures every
 *   gt tree of a pair has at least 5 points. */
enum { TL_EVAL_XY = 0, TL_EVAL_Z = 1 };
int tl_eval_partition(const double* xyz, const int64_t* gt, const int64_t* pred, int64_t n, const int64_t* gt_order, const int64_t* gt_start,
                      int64_t n_gt, const int64_t* pred_order, const int64_t* pred_start, int64_t n_pred, const int64_t* pairs, int64_t m,
                      const double* edges, int n_edges, int mode, int64_t* tp, int64_t* fp, int64_t* fn, double* norm, tl_stream_t stream);

/* ------------------------------------------------------------------ per-tree inventory of a labelled cloud (csrc/tl_inventory.hip)
 * Position, height, stem diameter at breast height and crown cells of every tree of a segmented forest, on the device.  The semantics
 * are the project's own (restated in numpy float64 in tests/inventory_restatement.py); all arithmetic is f64 in plain operators, no fma
 * contraction.  The caller sorts the labels once (stable) and keeps the rows of labels >= 1: tree t (label t + 1) is rows
 * start[t] .. start[t + 1] of the gathered cloud; an empty range is a tree without points.
 * tl_inventory_gather: out_xyz f64[n,3], row j = columns 0..2 of row order[j] of pts (f32 or f64 by dtype_f64, row stride ld >= 3
 *   elements, n_src rows), widened exactly; an index outside 0 .. n_src - 1 gives NaN.
 * tl_tree_inventory: one workgroup per tree.  table f64[n_trees, 10] = z_low, z_top, height, x, y, z, dbh, dbh_x, dbh_y, dbh_rmse;
 *   counts i64[n_trees, 2] = n_points, dbh_n.
 *   z_low = the 4th smallest z, rank 3 with duplicates counted (the tree-base rule of tl_train_item), for more than 11 rows, else the
 *   minimum; z_top = the 4th largest z for more than 11 rows, else the maximum; height = z_top - z_low.
 *   (x, y, z) = mean of the base rows, z <= z_low + 0.5.
 *   Slice rows: (z_low + slice_height) - slice_thickness / 2 <= z < (z_low + slice_height) + slice_thickness / 2 and w < dbh_max_radius^2,
 *   u = x_row - x, v = y_row - y, w = u*u + v*v; dbh_n = their number.  Algebraic (Kasa) circle fit:
 *   [[Suu, Suv, Su], [Suv, Svv, Sv], [Su, Sv, dbh_n]] [a, b, c]^T = [Suw, Svw, Sw] by Gaussian elimination with partial pivoting;
 *   cx = a / 2, cy = b / 2, r2 = (c + cx*cx) + cy*cy; dbh = 2 sqrt(r2), dbh_x = cx + x, dbh_y = cy + y,
 *   dbh_rmse = sqrt(sum((sqrt((u-cx)^2 + (v-cy)^2) - r)^2) / dbh_n).  These four are NaN when dbh_n < dbh_min_points, a pivot is below
 *   1e-12 times the largest matrix entry, or r2 <= 0.  A tree without rows has n_points = 0 and NaN in all ten columns.
 *   Sums: registers, a fixed wave butterfly, then the wave sums in wave order -- no float atomics, the same bits run to run.
 * tl_crown_keys: keys i64[n] = (label << 42) | ((floor(x / cell) + 2^20) << 21) | (floor(y / cell) + 2^20) per gathered row (sorted_label
 *   i64[n] = its label); *err (device) = 1 when a cell index is outside -2^20 .. 2^20 - 1 or a label outside 1 .. 2^21 - 1 (the key is
 *   then 0 and the caller raises), else 0.
 * tl_crown_count: cells i64[n_trees] (overwritten) = distinct keys of each tree among sorted_keys (ascending).  n_trees < 2^21.
 * A null or misaligned pointer, a negative size, slice_thickness <= 0, dbh_max_radius <= 0 or cell <= 0: TL_ERR_ARG, nothing launched.
 * n = 0 or n_trees = 0: TL_OK without a launch. */
int tl_inventory_gather(const void* pts, int dtype_f64, int64_t ld, int64_t n_src, const int64_t* order, int64_t n, double* out_xyz,
                        tl_stream_t stream);
int tl_tree_inventory(const double* sorted_xyz, int64_t n, const int64_t* start, int64_t n_trees, double slice_height, double slice_thickness,
                      double dbh_max_radius, int64_t dbh_min_points, double* table, int64_t* counts, tl_stream_t stream);
int tl_crown_keys(const double* sorted_xyz, const int64_t* sorted_label, int64_t n, double cell, int64_t* keys, int32_t* err,
                  tl_stream_t stream);
int tl_crown_count(const int64_t* sorted_keys, int64_t n, int64_t n_trees, int64_t* cells, tl_stream_t stream);

/* ------------------------------------------------------------------ terrain model of a labelled cloud (csrc/tl_terrain.hip)
 * A raster of ground heights (DTM) from the non-tree rows of a segmented forest, the ground under any point, and the per-tree columns
 * measured from that ground.  The semantics are the project's own (restated in numpy float64 in tests/terrain_restatement.py); all
 * arithmetic is f64 in plain operators, no fma contraction.  The grid is row-major [ny, nx], nx, ny <= 32768, nx * ny <= 2^26; a row's
 * cell is (floor(x / cell) - ix0, floor(y / cell) - iy0); the centre of cell i is ((ix0 + i) + 0.5) * cell.
 * tl_dtm_min: pts f32 or f64 by dtype_f64, row stride ld >= 3 elements, n rows, widened exactly; labels i64[n] or NULL.  Candidates are
 *   the rows with label 0 (every row when labels is NULL).  keys u64[ny, nx] (overwritten) = the order-preserving image of the lowest
 *   candidate z of the cell (sign bit set for z >= 0, all bits flipped for z < 0), all-ones for a cell without a candidate;
 *   n_candidates i32[ny, nx] (overwritten) = candidates per cell.  Integer atomics only: exact, the same bits for any row order.
 *   *err (device) = 1 when a coordinate is not finite or a row lies outside the grid (that row is skipped and the caller raises), else 0.
 * tl_dtm_filter: zmin f64[ny, nx] = the decoded minimum (NaN for a cell without one); state u8[ny, nx] = 0 empty, 2 rejected, 1 ground.
 *   A cell p with a minimum is rejected when another cell q with a minimum, within Chebyshev distance `window`, has
 *   zmin[p] - zmin[q] > max_slope * (cell * sqrt(di*di + dj*dj)) + step_tol (strict; evaluated against the raw minima, one pass).
 * tl_dtm_fill: z f64[ny, nx], state u8[ny, nx] from zmin / state_in (distinct buffers).  A ground cell keeps its minimum and state 1.
 *   Any other cell takes, at the first Chebyshev radius rho = 1 .. fill_radius whose window holds a ground cell, sum(w z) / sum(w) over
 *   the ground cells of that window in row-major order, w = 1 / (di*di + dj*dj), and state 3 (was empty) or 4 (was rejected); without
 *   such a radius NaN and its state (0 or 2).
 * tl_dtm_sample: per row, u = x / cell - (ix0 + 0.5), i0 = floor(u), fx = u - i0, i0 and i0 + 1 clamped to 0 .. nx - 1, the same in y;
 *   with four finite corners (g00 (1 - fx) + g10 fx) (1 - fy) + (g01 (1 - fx) + g11 fx) fy, else the value of the cell that contains
 *   the point (indices clamped), NaN included; NaN for a non-finite x or y or an empty grid.  ground f64[n] and / or hag f64[n] = z - ground
 *   (either may be NULL, not both; ld >= 2, >= 3 with hag).
 * tl_tree_ground (csrc/tl_inventory.hip): one workgroup per tree over the ranges of tl_tree_inventory, whose `table` it reads (z_low,
 *   z_top, x, y), with z_ground f64[n_trees] = the ground sampled at (x, y).  ground_table f64[n_trees, 7] = z_ground, height_ag =
 *   z_top - z_ground, base_gap = z_low - z_ground, dbh_ag, dbh_ag_x, dbh_ag_y, dbh_ag_rmse; ground_n i64[n_trees] = dbh_ag_n: the slice,
 *   fit and NaN rules of tl_tree_inventory with z_ground in place of z_low (the same device functions).  A NaN z_ground or a tree
 *   without rows: NaN in all seven, ground_n = 0.
 * A null or misaligned pointer, a negative size, a grid beyond the limits, cell <= 0, max_slope < 0, step_tol < 0, window < 0,
 * fill_radius < 0, slice_thickness <= 0 or dbh_max_radius <= 0: TL_ERR_ARG, nothing launched.  n = 0, n_trees = 0 or an empty grid:
 * TL_OK without a kernel launch. */
int tl_dtm_min(const void* pts, int dtype_f64, int64_t ld, int64_t n, const int64_t* labels, double cell, int64_t ix0, int64_t iy0, int nx, int ny,
               uint64_t* keys, int32_t* n_candidates, int32_t* err, tl_stream_t stream);
int tl_dtm_filter(const uint64_t* keys, int nx, int ny, double cell, double max_slope, double step_tol, int window, double* zmin, uint8_t* state,
                  tl_stream_t stream);
int tl_dtm_fill(const double* zmin, const uint8_t* state_in, int nx, int ny, int fill_radius, double* z, uint8_t* state, tl_stream_t stream);
int tl_dtm_sample(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* z, double cell, int64_t ix0, int64_t iy0, int nx, int ny,
                  double* ground, double* hag, tl_stream_t stream);
int tl_tree_ground(const double* sorted_xyz, int64_t n, const int64_t* start, int64_t n_trees, const double* table, const double* z_ground,
                   double slice_height, double slice_thickness, double dbh_max_radius, int64_t dbh_min_points, double* ground_table,
                   int64_t* ground_n, tl_stream_t stream);

/* ------------------------------------------------------------------ stem profiles of a labelled cloud (csrc/tl_stem.hip)
 * A circle per horizontal slab along every stem, tracked bottom-up, and from the accepted circles the stem volume, the diameter at breast
 * height, the lean and the taper.  The semantics are the project's own and have no reference call site: tests/stem_restatement.py
 * restates them in numpy float64.  All arithmetic is f64 in plain operators, no fma contraction; distances are compared squared.
 * The rows are those of tl_inventory_gather (label order, sorted_label i64[n] = the label of each, tree t = label t + 1);
 * tree f64[n_trees, 4] = px, py, z_ref, z_top per tree: the inventory's position and z_top, and z_low or z_ground as the reference.
 * Slab k of a tree exists when k < max_slices and h_k = first_height + k * step <= z_top - z_ref (none for a NaN); zc_k = z_ref + h_k,
 * lo_k = zc_k - thickness / 2, hi_k = zc_k + thickness / 2.  S, the profile width, is the largest slab count of any tree (the caller's).
 * tl_stem_keys: keys i64[n]: tree * S + k for a row with (x - px)^2 + (y - py)^2 < corridor^2 that lies in slab k, lo_k <= z < hi_k (the
 *   lowest such k; found among floor(q) - 1 .. floor(q) + 1, q = ((z - z_ref) - (first_height - thickness / 2)) / step, by the exact
 *   rule), else the sentinel n_trees * S: also for a label outside 1 .. n_trees, a non-finite value or a q outside (-2, max_slices + 1).
 *   The caller sorts the keys (stable), gathers the rows below the sentinel in key order (stem_xyz, n rows) and takes
 *   slab_start i64[n_trees * S + 1] = the first row of every key.
 * tl_stem_profile: one workgroup per tree walks k = 0 .. with c = (px, py), R = start_radius, r_prev = NaN, misses = 0.  A slab after the
 *   walk stopped: state 0, n = 0.  Otherwise n = the slab's rows with u*u + v*v < R*R, u = x - c.x, v = y - c.y; with n >= min_points the
 *   circle fit of tl_tree_inventory on (u, v) (the same device functions), rmse = sqrt(sum((sqrt(du*du + dv*dv) - r)^2) / n).  Accepted
 *   (state 1) when the fit succeeded, rmse <= max_rmse, min_radius <= r <= max_radius and r <= max_growth * r_prev (or r_prev is NaN):
 *   x = cx + c.x, y = cy + c.y, then c = (x, y), r_prev = r, R = search_factor * r + search_margin, misses = 0.  Otherwise state 2,
 *   misses += 1, and the walk stops at misses >= max_misses.
 *   profile f64[n_trees, S, 5] = h, x, y, r, rmse (NaN in the last four unless accepted; h = NaN for a slab the tree does not have);
 *   pcount i64[n_trees, S, 2] = n, state; slices i64[n_trees] = accepted slabs m; summary f64[n_trees, 6], over them in ascending k:
 *   stem_base_h, stem_top_h = h of the first / last; stem_volume = (PI * (r0 * r0)) * h_first, then for every consecutive accepted pair
 *   V = V + ((PI / 3.0) * (h_j - h_i)) * ((r_i * r_i + r_i * r_j) + r_j * r_j); dbh_stem = 2.0 * (r_i + (r_j - r_i) * ((dbh_height - h_i)
 *   / (h_j - h_i))) for the first such pair with h_i <= dbh_height <= h_j, else NaN; stem_lean = atan2(sqrt(dx*dx + dy*dy), h_last -
 *   h_first) * (180.0 / PI), (dx, dy) = last centre - first centre; stem_taper = sum((h - hm)(d - dm)) / sum((h - hm)^2), d = 2.0 * r,
 *   hm = sum(h) / m, dm = sum(d) / m.  All six NaN for m = 0, lean and taper NaN for m < 2.
 *   Sums: registers, a fixed wave butterfly, then the wave sums in wave order -- no float atomics, the same bits run to run.
 * A null or misaligned pointer, a negative size, S > max_slices or a parameter outside its constraint (first_height, step, corridor,
 * start_radius, max_rmse, dbh_height > 0; 0 < thickness <= step; max_slices in 1 .. 256; search_factor, max_growth >= 1; search_margin
 * >= 0; min_points >= 3; 0 < min_radius <= max_radius; max_misses >= 1; all finite): TL_ERR_ARG, nothing launched.  n_trees = 0 or S = 0,
 * and tl_stem_keys with n = 0: TL_OK without a launch (outputs untouched).  tl_stem_profile with n = 0 rows
 * still walks every tree: each visited slab is a miss. */
typedef struct tl_stem_params {
  double first_height, step, thickness, corridor, start_radius, search_factor, search_margin, max_rmse, min_radius, max_radius, max_growth,
      dbh_height;
  int64_t max_slices, min_points, max_misses;
} tl_stem_params;
int tl_stem_keys(const double* sorted_xyz, const int64_t* sorted_label, int64_t n, const double* tree, int64_t n_trees, int64_t S,
                 const tl_stem_params* params, int64_t* keys, tl_stream_t stream);
int tl_stem_profile(const double* stem_xyz, int64_t n, const int64_t* slab_start, const double* tree, int64_t n_trees, int64_t S,
                    const tl_stem_params* params, double* profile, int64_t* pcount, double* summary, int64_t* slices, tl_stream_t stream);

/* ------------------------------------------------------------------ crown structure of a labelled cloud (csrc/tl_crown.hip)
 * Where the crown of every tree begins, how many voxels it fills, the cells it projects onto the ground and its radius in eight
 * directions, on a grid of cell x cell x layer.  The semantics are the project's own and have no reference call site:
 * tests/crown_restatement.py restates them in numpy float64.  All arithmetic is f64 in plain operators, no fma contraction; every other
 * quantity is an integer count.  The rows and `tree` f64[n_trees, 4] = px, py, z_ref, z_top are those of the stem profiles above.
 * H = z_top - z_ref; L_t = min(floor(H / layer) + 1, max_layers), 0 unless H >= 0 (NaN: none).  A row is in layer l = floor((z - z_ref) /
 * layer) when 0 <= l < L_t, in cell (ix, iy) = (floor(x / cell), floor(y / cell)).
 * tl_crown_voxel_keys: keys i64[n] = (t << 34) | (ix_rel << 21) | (iy_rel << 8) | l for a row of tree t = label - 1 in layer l, ix_rel =
 *   ix - floor(px / cell) + 4096, the same in y; else the sentinel 2^55: a label outside 1 .. n_trees or a row in no layer.  *err
 *   (device) = 1 when a row of a label in 1 .. n_trees has a coordinate that is not finite, or a row in a layer has ix_rel or iy_rel
 *   outside 0 .. 8191 (the row gets the sentinel and the caller raises), else 0.  Every range is tested on the f64 value.
 *   The caller sorts the keys and takes kstart i64[n_trees + 1]: kstart[t] = the first key >= t << 34.
 * tl_crown_structure: one workgroup per tree over sorted_keys[kstart[t] .. kstart[t + 1]).  n[l] = its keys of layer l, cells[l] = the
 *   distinct ones.  l_min = the smallest l with l * layer >= min_height (counted up from 0, at most max_layers).  With l_min < L_t and a
 *   row in a layer >= l_min: cells_max = max cells[l] over l_min <= l < L_t, l_w the lowest l that reaches it; l_b = l_w, gap = 0, then for
 *   l = l_w - 1 down to l_min: cells[l] * 100 >= base_percent * cells_max: l_b = l, gap = 0; else gap += 1 and stop at gap > max_gap.
 *   A projection cell is an (ix, iy) with a key in a layer >= l_b; with c = their number, (sx, sy) = the integer sums of ix, iy over them:
 *   u = (ix + 0.5) * cell - px, v likewise, w = u*u + v*v; sector 0 .. 7 of (u, v) counter-clockwise from +x by comparisons (u > 0, v >= 0:
 *   v < u ? 0 : 1; u <= 0, v > 0: -u < v ? 2 : 3; u < 0, v <= 0: -v < -u ? 4 : 5; u >= 0, v < 0: u < -v ? 6 : 7; u = v = 0: 0).
 *   counts i64[n_trees, 3] = crown_layers (L_t), crown_voxels (sum of cells[l], l >= l_b), crown_proj_cells (c);
 *   summary f64[n_trees, 11] = crown_base_h (l_b * layer), crown_length (H - base), crown_ratio (length / H), crown_widest_h ((l_w + 0.5) *
 *   layer), crown_volume (voxels * ((cell * cell) * layer)), crown_proj_area (c * (cell * cell)), crown_x, crown_y (((sx / c) + 0.5) *
 *   cell), crown_offset (sqrt(dx*dx + dy*dy), dx = crown_x - px), crown_radius_max, crown_radius_mean (the sum of the eight in sector
 *   order / 8.0); radii f64[n_trees, 8] = sqrt(max w) per sector, 0.0 for an empty one.  A tree without a crown: NaN in summary and
 *   radii, 0 in voxels and cells.  prof_h f64[n_trees, L] = l * layer, pcount i64[n_trees, L, 2] = n[l], cells[l] for l < L_t, else NaN,
 *   0, 0; L >= every L_t is the caller's (layers beyond L are not written).  Fewer than 2^32 rows per tree and layer.
 *   Counts are integer adds in LDS, the sums integers, the maxima exact: the same bits run to run and for any row order.
 * A null or misaligned pointer, a negative size, n_trees >= 2^21, L > max_layers or a parameter outside its constraint (layer, cell > 0,
 * min_height >= 0, all finite; max_layers in 1 .. 256; base_percent in 1 .. 100; max_gap >= 0): TL_ERR_ARG, nothing launched.  Then
 * n = 0 or n_trees = 0 (tl_crown_voxel_keys) and n_trees = 0 or L = 0 (tl_crown_structure): TL_OK without a launch, outputs and *err
 * untouched. */
typedef struct tl_crown_params {
  double layer, cell, min_height;
  int64_t max_layers, base_percent, max_gap;
} tl_crown_params;
int tl_crown_voxel_keys(const double* sorted_xyz, const int64_t* sorted_label, int64_t n, const double* tree, int64_t n_trees,
                        const tl_crown_params* params, int64_t* keys, int32_t* err, tl_stream_t stream);
int tl_crown_structure(const int64_t* sorted_keys, int64_t n, const int64_t* kstart, const double* tree, int64_t n_trees, int64_t L,
                       const tl_crown_params* params, double* summary, int64_t* counts, double* prof_h, int64_t* pcount, double* radii,
                       tl_stream_t stream);

/* ------------------------------------------------------------------ branch structure of a labelled cloud (csrc/tl_skeleton.hip)
 * What is inside the crown: the geodesic distance of every voxel of a tree from its stem base along the tree's own voxels, the level sets
 * of that distance cut into connected components (the skeleton nodes) and every node's parent.  The semantics are the project's own and
 * have no reference call site: tests/branches_restatement.py restates them in Python.  Every result but the node centroids is an integer;
 * the f64 arithmetic (floor(coordinate / voxel), the centroid division) is in plain operators, no fma contraction.  The rows and `tree`
 * f64[n_trees, 4] = px, py, z_ref, z_top are those of the crown structure above.
 * A voxel is (ix, iy, iz) = floor((x, y, z) / voxel), one grid for all trees; (ipx, ipy, izr) = floor((px, py, z_ref) / voxel).
 * tl_skel_voxel_keys: keys i64[n] = (t << 35) | (ix_rel << 23) | (iy_rel << 11) | iz_rel for a row of tree t = label - 1, ix_rel = ix - ipx +
 *   2048, the same in y, iz_rel = iz - izr; else -1: a label outside 1 .. n_trees, a tree whose px, py or z_ref is not finite, or a row
 *   with iz < izr.  *err (device) = 1 when a row of a label in 1 .. n_trees has a coordinate that is not finite, or a row with iz >= izr
 *   has |ix - ipx| > 2047, |iy - ipy| > 2047 or iz_rel >= 2047 (the row gets -1 and the caller raises), else 0.  Every range is tested on
 *   the f64 value.  The caller sorts the keys, drops the repeats and the -1, and takes kstart i64[n_trees + 1]: kstart[t] = the first key
 *   >= t << 35.  voxel_keys i64[n] below are those distinct ascending keys; a voxel is its index (n < 2^31), and index order is key order.
 * The graph: an edge joins two voxels of one tree with max(|dx|, |dy|, |dz|) <= reach, of weight floor(sqrt(10000 * (dx^2 + dy^2 + dz^2))):
 *   100, 141, 173 (reach 1), 200, 223, 244, 282, 300, 346 (reach 2).  Neighbours are looked up inside [kstart[t], kstart[t + 1]) only.
 * tl_skel_distance: one workgroup per tree.  Sources: of the voxels with |ix_rel - 2048|, |iy_rel - 2048| <= base_reach, those fewer than
 *   base_layers above the lowest of them.  d i32[n] = the shortest-path distance from the source set, 0 on sources, -1 for a voxel no path
 *   reaches, for every voxel of a tree without a source and of a tree of more than max_voxels voxels.  rounds i32[n_trees] = the number
 *   of bucket rounds the tree took (0 without a skeleton).  The distance is unique: the same bits whatever the order of the atomics.
 * tl_skel_nodes: bin(v) = d(v) / (100 * level).  A node is a connected component, under the edges above, of reached voxels of one bin.
 *   parent i32[n] (overwritten) = a union-find forest whose roots are the nodes' smallest voxels; acc i64[n, 4] (overwritten) = at a root:
 *   the node's voxels, the sums of their ix_rel, iy_rel, iz_rel, elsewhere 0; vstar i64[n] (overwritten) = at a root: (d << 32) | index of
 *   the node's voxel with the smallest (d, key), elsewhere -1.
 * tl_skel_links: one thread per node.  roots i32[n_nodes] = the root voxels in the caller's node order (tree, bin, root ascending),
 *   node_id i32[n] = the node's index in that order at a root, node_start i64[n_trees + 1] = the first node of every tree.  node_xyz
 *   f64[n_nodes, 3] = ((double)sum / (double)count + 0.5) * voxel per axis, the sums taken to absolute voxel indices in integers;
 *   node_bin i32, node_count i64; node_parent i32 = -1 for a node of bin 0, else the node (index local to the tree) of the predecessor of
 *   the node's first voxel v*: its neighbour u with d(u) + w(u, v*) = d(v*) of the smallest key.  It has a smaller bin.
 * A null or misaligned pointer, a negative size, n >= 2^31, n_nodes > n, n_trees >= 2^21 or a parameter outside its constraint (voxel > 0,
 * min_branch, min_height >= 0, all finite; reach 1 or 2; base_reach in 0 .. 2047; base_layers >= 1; level in 1 .. 10^6; max_voxels >= 1):
 * TL_ERR_ARG, nothing launched.  Then n = 0 or n_trees = 0 (and n_nodes = 0 for tl_skel_links): TL_OK without a launch, outputs and *err
 * untouched.  d stays below 2^31 for max_voxels <= 2^22 (346 per step), which util.branches enforces. */
typedef struct tl_skel_params {
  double voxel, min_branch, min_height;
  int64_t reach, base_reach, base_layers, level, max_voxels;
} tl_skel_params;
int tl_skel_voxel_keys(const double* sorted_xyz, const int64_t* sorted_label, int64_t n, const double* tree, int64_t n_trees,
                       const tl_skel_params* params, int64_t* keys, int32_t* err, tl_stream_t stream);
int tl_skel_distance(const int64_t* voxel_keys, int64_t n, const int64_t* kstart, int64_t n_trees, const tl_skel_params* params, int32_t* d,
                     int32_t* rounds, tl_stream_t stream);
int tl_skel_nodes(const int64_t* voxel_keys, int64_t n, const int64_t* kstart, int64_t n_trees, const tl_skel_params* params, const int32_t* d,
                  int32_t* parent, int64_t* acc, int64_t* vstar, tl_stream_t stream);
int tl_skel_links(const int64_t* voxel_keys, int64_t n, const int64_t* kstart, const double* tree, int64_t n_trees,
                  const tl_skel_params* params, const int32_t* d, int32_t* parent, const int64_t* acc, const int64_t* vstar, const int32_t* roots,
                  int64_t n_nodes, const int32_t* node_id, const int64_t* node_start, double* node_xyz, int32_t* node_parent, int32_t* node_bin,
                  int64_t* node_count, tl_stream_t stream);

/* ------------------------------------------------------------------ cylinder model of the skeleton (csrc/tl_wood.hip)
 * How thick the wood is: one Kasa circle fit per skeleton node of the branch structure above, in the plane across the node's axis.  The
 * semantics are the project's own (restated in Python in tests/wood_restatement.py); all arithmetic is f64 in plain operators, no fma
 * contraction.  The radii along the branches, the frusta and the columns are read off the node table on the host (util/wood.py).
 * tl_wood_row_nodes: one thread per gathered row.  row_keys i64[m] = the keys tl_skel_voxel_keys gave the rows; voxel_keys i64[n_voxels], d
 *   i32[n_voxels], uf_parent i32[n_voxels] (the union-find forest of tl_skel_nodes; read, paths are not compressed) and node_id
 *   i32[n_voxels] (the node of a root voxel) as tl_skel_links takes them.  row_node i32[m] = the node (global index) of the row's voxel when
 *   the key is >= 0, is found in voxel_keys and that voxel is reached (d >= 0); else -1.
 * The caller sorts row_node stably: perm i64[m] = the permutation, range_start i64[n_nodes + 1]: range_start[i] = the first position of the
 *   sorted values that is >= i, so that perm[range_start[i] .. range_start[i + 1]) are the rows of node i.
 * tl_wood_fit: one wavefront per node.  node_xyz f64[n_nodes, 3], node_parent i32[n_nodes] (local to the tree, -1 for a root), node_start
 *   i64[n_trees + 1] are the node table of tl_skel_links.  Axis a: for a node with a parent at the centroid distance seg = sqrt(dx dx + dy dy
 *   + dz dz) > 0: (c - c_parent) / seg; else (0, 0, 1).  Basis: k = the index of the smallest |a_k| (the first among equals), w = a x e_k,
 *   e1 = w / |w|, e2 = a x e1.  Over the node's rows p: q = p - c, u = q . e1, v = q . e2.  n = the rows; with n >= min_points the Kasa
 *   circle (cu, cv, r) of the (u, v) and rmse = sqrt(sum((sqrt((u - cu)^2 + (v - cv)^2) - r)^2) / n).  The fit is accepted when the solve
 *   succeeded, min_radius <= r <= max_radius, rmse <= max_rmse and sqrt(cu^2 + cv^2) <= r.  state i32[n_nodes] = 0 for n < min_points, 1
 *   accepted, 2 rejected; count i64[n_nodes] = n; radius_fit, rmse f64[n_nodes] and centre f64[n_nodes, 3] = c + cu e1 + cv e2 are NaN
 *   unless state is 1; axis f64[n_nodes, 3] = a.  Sums: lane l of 64 adds the rows l, l + 64, ... of the node's range in that order,
 *   then a fixed xor butterfly: the same bits for the same permutation.  max_growth and dbh_height are the host rules' (util/wood.py).
 * A null or misaligned pointer, a negative size, n_voxels or n_nodes >= 2^31, n_nodes > n_voxels (tl_wood_row_nodes) or a parameter outside
 * its constraint (min_points >= 3; max_rmse >= 0; 0 <= min_radius < max_radius; max_growth >= 1; dbh_height >= 0; all finite): TL_ERR_ARG,
 * nothing launched.  Then m = 0 or n_nodes = 0 (or n_trees = 0 for tl_wood_fit): TL_OK without a launch, outputs untouched. */
typedef struct tl_wood_params {
  double max_rmse, min_radius, max_radius, max_growth, dbh_height;
  int64_t min_points;
} tl_wood_params;
int tl_wood_row_nodes(const int64_t* row_keys, int64_t m, const int64_t* voxel_keys, int64_t n_voxels, const int32_t* d, int32_t* uf_parent,
                      const int32_t* node_id, int64_t n_nodes, int32_t* row_node, tl_stream_t stream);
int tl_wood_fit(const double* sorted_xyz, int64_t m, const int64_t* perm, const int64_t* range_start, const double* node_xyz,
                const int32_t* node_parent, const int64_t* node_start, int64_t n_trees, int64_t n_nodes, const tl_wood_params* params,
                double* radius_fit, int64_t* count, double* rmse, int32_t* state, double* centre, double* axis, tl_stream_t stream);

/* ------------------------------------------------------------------ leaf-wood separation of a labelled cloud (csrc/tl_leafwood.hip)
 * Which rows of a tree are wood: a seed rule on the eigen-features above, then a spatial vote over the same radius neighbourhoods among
 * the rows of the same tree.  The semantics are the project's own (restated in numpy in tests/leafwood_restatement.py).  The connectivity
 * filter behind the vote reuses tl_skel_voxel_keys, tl_skel_nodes and tl_wood_row_nodes (util/leafwood.py).
 * tl_leafwood_seed: one thread per row.  feats f32[n, 4] = linearity, planarity, verticality, number_of_neighbors of tl_eigen_features
 *   (ids 5, 4, 10, 14) at `radius`.  flag u8[n] = 1 when number_of_neighbors >= min_neighbours, the three features are finite and
 *   (linearity >= linearity_min, or planarity >= planarity_min and verticality >= verticality_min); else 0.  The f32 values are widened
 *   to f64 and compared with the f64 thresholds; NaN gives 0.
 * tl_leafwood_vote: one synchronous round.  xyz_sorted, sorted_keys, extent2, piece_start and n_pieces as tl_eigen_features takes them
 *   (cells of `radius`); tag i32[n] in sorted order = (tree << 1) | flag of the round before, tree >= 0.  For a row p: a = the rows q of
 *   the same tree with dx dx + dy dy + dz dz <= radius radius (f64, this expression, no contraction; p included), w = those of them
 *   whose flag is 1; flag_out u8[n] = 1 exactly when 100 w >= vote_percent a, in integers; tag_out i32[n] = (tree << 1) | flag_out, the
 *   tag of the next round (may be NULL; must not be tag).  Counts only: the same bits for any row order and any piece table.  One
 *   wave per piece; a row whose piece is missing from the table is not written.  One launch, no atomics.
 * A null or misaligned pointer, n or n_pieces < 0, n_pieces > n or > 2^31 - 1, extent2 outside 0 .. 2^21 - 1, tag_out == tag or a
 * parameter outside its constraint (radius, voxel > 0 and finite; min_neighbours >= 3; the three thresholds in [0, 1]; vote_iters in
 * 0 .. 8; vote_percent in 1 .. 100; reach 1 or 2; min_component >= 1; filter 0 or 1; NaN fails every one): TL_ERR_ARG, nothing launched.
 * Then n = 0 (or n_pieces = 0 for tl_leafwood_vote): TL_OK without a launch, outputs untouched.  vote_iters, voxel, reach,
 * min_component and filter are the host's (util/leafwood.py). */
typedef struct tl_leafwood_params {
  double radius, linearity_min, planarity_min, verticality_min, voxel;
  int64_t min_neighbours, vote_iters, vote_percent, reach, min_component, filter;
} tl_leafwood_params;
int tl_leafwood_seed(const float* feats, int64_t n, const tl_leafwood_params* params, uint8_t* flag, tl_stream_t stream);
/* tl_leafwood_seed_scales: the seed over S scales, one thread per row.  feats f32[n, S, 4] = the four columns of
 *   tl_leafwood_seed as tl_eigen_features_scales writes them (16-byte aligned).  The rule of tl_leafwood_seed is applied to every
 *   scale on its own (a scale with fewer than min_neighbours neighbours or a NaN does not hold); flag u8[n] = 1 exactly when at least
 *   scales_min scales hold.  With S = 1 and scales_min = 1 it is tl_leafwood_seed.  TL_ERR_ARG, nothing launched: whatever
 *   tl_leafwood_seed refuses, S outside 1 .. TL_FEAT_MAX_SCALES, scales_min outside 1 .. S.  n = 0: TL_OK without a launch. */
int tl_leafwood_seed_scales(const float* feats, int64_t n, int S, const tl_leafwood_params* params, int scales_min, uint8_t* flag,
                            tl_stream_t stream);
int tl_leafwood_vote(const double* xyz_sorted, const int64_t* sorted_keys, int64_t n, const int64_t* extent2, const int64_t* piece_start,
                     int64_t n_pieces, const int32_t* tag, const tl_leafwood_params* params, uint8_t* flag_out, int32_t* tag_out,
                     tl_stream_t stream);

/* ------------------------------------------------------------------ canopy height model of a cloud (csrc/tl_canopy.hip)
 * The per-area side of the measurements: the highest height above ground per cell (CHM) with pits and holes mended, tree tops on it,
 * and height statistics per cell of a coarser metrics grid.  The semantics are the project's own (restated in numpy float64 in
 * tests/canopy_restatement.py); all arithmetic is f64 in plain operators, no fma contraction.  Grids follow the terrain's rule: row-major
 * [ny, nx], nx, ny <= 32768, nx * ny <= 2^26, a row's cell is (floor(x / cell) - ix0, floor(y / cell) - iy0).  pts f32 or f64 by dtype_f64,
 * row stride ld >= 2 elements (x, y are read), n rows, widened exactly; h f64[n] = the height above ground of each row.  A row whose h is
 * NaN takes part in nothing.  -0.0 counts as 0.0.
 * tl_chm_max: keys u64[ny, nx] (overwritten) = the order-preserving image of the highest h of the cell (sign bit set for h >= 0, all bits
 *   flipped for h < 0), 0 for a cell without a row; count i32[ny, nx] (overwritten) = its rows with a finite h.  flags i32[2] (device,
 *   overwritten): flags[0] = 1 when an x or y is not finite, an h is infinite or a row lies outside the grid (the row is skipped and the
 *   caller raises), else 0; flags[1] = the rows whose h is NaN.  Integer atomics only: exact, the same bits for any row order.
 * tl_chm_owner: owner i32[ny, nx] (overwritten) = the largest label among the rows whose h equals the decoded keys[cell], -1 for a cell
 *   without a row (or whose tying rows all have labels below 0); labels i64[n], read for the tying rows only.  *err (device) is set to 1
 *   for a tying label outside the i32 range and is otherwise left as it is.
 * tl_chm_pits: top f64[ny, nx] = the decoded maximum (NaN for an empty cell).  Per cell, v = the non-NaN tops among its 8 neighbours
 *   inside the grid, k their number, m their median: sorted ascending, v[k / 2] for odd k, (v[k / 2 - 1] + v[k / 2]) / 2.0 for even k.
 *   state u8 / chm f64[ny, nx]: a cell with rows, k >= pit_min_neighbours and m - top > pit_depth (strict): 2, m; any other cell with rows:
 *   1, top; an empty cell with k >= pit_min_neighbours: 3, m; any other empty cell: 0, NaN.  One pass against the raw tops.
 * tl_chm_tops: mask u8[ny, nx] = 1 for a cell whose chm is not NaN and >= min_height, when no cell within Chebyshev distance `window`
 *   (clipped to the grid) has a greater chm and none of them with an equal chm has a smaller row-major index; else 0.
 * tl_canopy_keys: keys i64[n] = the row-major index of the row's cell, -1 for a row whose h is NaN.  *err (device) is set to 1 when an x
 *   or y is not finite, an h is infinite or a row lies outside the grid (the row gets -1), and is otherwise left as it is.
 * tl_grid_metrics: one workgroup per cell over sorted_h[start[c] .. start[c + 1]): the heights of the cell's rows in ascending order
 *   (start i64[cells + 1], ascending, within 0 .. n).  With r = the rows of the range, m = those with h > cutoff (strict; they are the
 *   last m of the range, v[0 .. m)): counts i32[cells, 2] = r, m; metrics f64[cells, 4 + n_percentiles] = cover (m / r as doubles),
 *   h_max (the last value), h_mean = sum(v) / m, h_sd = sqrt(sum((v - h_mean)^2) / m), then per percentile q (host array of
 *   n_percentiles values in [0, 100], 1 .. 16 of them): pos = (q / 100.0) * (m - 1), lo = floor(pos), t = pos - lo, v[lo] + (v[min(lo + 1,
 *   m - 1)] - v[lo]) * t.  NaN in all of them for r = 0, in all but cover and h_max for m = 0.  layers i32[cells, L]: a row with h < 0
 *   counts in layer 0, any other in layer min(floor(h / layer), L - 1); *n_clipped (device, overwritten) = the rows of all cells with h >=
 *   L * layer.  Sums: thread t of 256 adds v[t], v[t + 256], ... in that order, then a fixed pairwise tree over the 256 partial sums: the
 *   same bits for the same sorted values.
 * A null or misaligned pointer, a negative size, a grid beyond the limits, cell <= 0, pit_depth < 0, pit_min_neighbours outside 1 .. 9,
 * window < 1, layer <= 0, L outside 1 .. 256, n_percentiles outside 1 .. 16, a percentile outside [0, 100] or a value that is not finite:
 * TL_ERR_ARG, nothing launched.  Then n = 0 (the row passes), an empty grid or cells = 0: TL_OK without a kernel launch; tl_chm_max and
 * tl_chm_owner still clear keys, count, flags and owner, tl_grid_metrics *n_clipped. */
int tl_chm_max(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* h, double cell, int64_t ix0, int64_t iy0, int nx, int ny,
               uint64_t* keys, int32_t* count, int32_t* flags, tl_stream_t stream);
int tl_chm_owner(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* h, const int64_t* labels, double cell, int64_t ix0,
                 int64_t iy0, int nx, int ny, const uint64_t* keys, int32_t* owner, int32_t* err, tl_stream_t stream);
int tl_chm_pits(const uint64_t* keys, int nx, int ny, double pit_depth, int pit_min_neighbours, double* top, double* chm, uint8_t* state,
                tl_stream_t stream);
int tl_chm_tops(const double* chm, int nx, int ny, int window, double min_height, uint8_t* mask, tl_stream_t stream);
int tl_canopy_keys(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* h, double cell, int64_t ix0, int64_t iy0, int nx, int ny,
                   int64_t* keys, int32_t* err, tl_stream_t stream);
int tl_grid_metrics(const double* sorted_h, int64_t n, const int64_t* start, int64_t cells, double cutoff, const double* percentiles,
                    int n_percentiles, double layer, int L, double* metrics, int32_t* counts, int32_t* layers, int32_t* n_clipped,
                    tl_stream_t stream);

/* ------------------------------------------------------------------ light under the canopy (csrc/tl_light.hip)
 * A bit grid of the occupied voxels of a cloud and a ray march through it: per origin and zenith ring, how the rays of a direction table
 * end.  The semantics are the project's own (restated in numpy float64 in tests/light_restatement.py); all arithmetic is f64 in plain
 * operators, no fma contraction; the only atomics are integer ones, so every output has the same bits for any row order.
 * The grid follows the terrain's rule in three axes: a row's voxel is (floor(x / voxel) - ix0, floor(y / voxel) - iy0, floor(z / voxel) -
 * iz0); nx, ny, nz <= 8192 and nx * ny * nz <= 2^31 without an owner grid, <= 2^28 with one.  occ u32[nz, ny, ceil(nx / 32)]: bit ix % 32
 * of word ix / 32 of row (iz, iy).  owner i32[nz, ny, nx].
 * tl_light_voxels: pts f32 or f64 by dtype_f64, row stride ld >= 3 elements, n rows, widened exactly.  occ (overwritten) gets the bit of
 *   every row's voxel.  labels i64[n] and owner go together, both given or both null: owner (overwritten) = the largest label >= 0 among
 *   the voxel's rows, -1 for a voxel without one.  *err (device, overwritten) = 1 when a coordinate is not finite, a row lies outside the
 *   grid or a label is outside the i32 range (the row is skipped and the caller raises), else 0.
 * tl_light_march: origins f64[n_origins, 3], skip i32[n_origins] or null (-1 for all), dirs f64[n_dirs, 3] (the host checks that they are
 *   finite and of unit length), ring i32[n_dirs] in 0 .. n_rings - 1 (a ray whose ring is outside that range is counted nowhere).  For
 *   origin o and direction d: i_a = floor(o_a / voxel) - i0_a per axis; an origin outside the grid (a NaN included) gets status 1 and no
 *   counts, any other status 0.  s_a = the sign of d_a; t_a = ((i0_a + i_a + (s_a > 0 ? 1 : 0)) * voxel - o_a) / d_a for s_a != 0, +inf
 *   for s_a = 0, always from the integer index.  Repeat: take the axis of the smallest t (ties to x, then y, then z), t_enter = t_a; if
 *   t_enter > max_range exit with code 2; i_a += s_a; if the index left the grid exit with code 1 through the top (a = z, s > 0) and 3
 *   through a side or the bottom; recompute t_a from the new index; the voxel entered is a hit when its bit is set and (skip < 0 or there
 *   is no owner grid or owner != skip); at min_hits hits exit with code 0 and first = t_enter.  The origin's own voxel is never tested.
 *   counts i32[n_origins, n_rings, 4] (overwritten): the rays of the origin and ring per exit code.  status i32[n_origins].  code
 *   u8[n_origins, n_dirs] or null (255 for an origin outside the grid); first f64[n_origins, n_dirs] or null (NaN unless the code is 0).
 *   One wave serves 64 consecutive directions of one origin; a lane's walk is bounded by nx + ny + nz steps.
 * A null or misaligned pointer, a negative size, ld < 3, a voxel that is not positive and finite, a grid beyond the limits, rows or
 * origins with an empty grid, n_rings outside 1 .. 65536, min_hits < 1, a max_range that is not positive and finite: TL_ERR_ARG, nothing
 * touched.  Then n = 0 or n_origins = 0: TL_OK without a kernel launch; tl_light_voxels still clears occ, owner and *err. */
int tl_light_voxels(const void* pts, int dtype_f64, int64_t ld, int64_t n, const int64_t* labels, double voxel, int64_t ix0, int64_t iy0,
                    int64_t iz0, int nx, int ny, int nz, uint32_t* occ, int32_t* owner, int32_t* err, tl_stream_t stream);
int tl_light_march(const double* origins, const int32_t* skip, int64_t n_origins, const double* dirs, const int32_t* ring, int64_t n_dirs,
                   int n_rings, const uint32_t* occ, const int32_t* owner, double voxel, int64_t ix0, int64_t iy0, int64_t iz0, int nx, int ny,
                   int nz, double max_range, int min_hits, int32_t* counts, int32_t* status, uint8_t* code, double* first, tl_stream_t stream);

/* ------------------------------------------------------------------ pictures of clouds and rasters (csrc/tl_render.hip)
 * Orthographic point splats with a depth test, rasters as depth-keyed pixels, and a shading pass.  The semantics are the project's own
 * (restated in numpy float64 in tests/render_restatement.py); all arithmetic is f64 in plain operators, no fma contraction, no
 * transcendental function; the only atomics are integer maxima, so every output has the same bits for any row order.
 * The canvas is keys u64[height, width], width and height in 1 .. 16384, image row 0 at the top; key 0 is an empty pixel.  A key is
 * image << 32 | rgb: rgb = r << 16 | g << 8 | b, image = the order-preserving u32 image of a float32 depth (bits ^ 0xFFFFFFFF when the
 * sign bit is set, else bits | 0x80000000; no finite or infinite depth maps to 0).  A larger depth is nearer the viewer and wins; equal
 * depths are settled by the larger rgb.
 * tl_splat: pts f32 or f64 by dtype_f64, row stride ld >= 3 elements, n rows, widened exactly.  views f64[n_views, 18] (device): u[3]
 *   screen right, v[3] screen up, w[3] towards the viewer, c[3] the centre, s pixels per metre, x0, y0, vw, vh the viewport on the
 *   canvas (integers held in f64, inside the canvas: the caller checks that), one reserved 0.  vid i32[n] or null (every row in view 0):
 *   a negative vid skips the row, a vid >= n_views skips it and sets flags[0].  q = p - c; a = (u0 * qx + u1 * qy) + u2 * qz, b and d
 *   likewise with v and w; px = floor(a * s + (x0 + vw / 2)), py = floor((y0 + vh / 2) - b * s); depth = float32(d + 0.0), round to
 *   nearest even.  A row with a coordinate that is not finite, or a depth that is not finite as float32, is skipped and sets flags[0].
 *   The footprint of `size` = k in 1 .. 9 is px - (k - 1) / 2 .. px + k / 2 and the same in y (integer divisions); each of its pixels
 *   inside the row's viewport (and the canvas) takes atomicMax(keys, key).  keys is NOT cleared: layers accumulate, the caller clears
 *   once.  flags i32[4] (device): flags[0] is set to 1 as said and otherwise left as it is; flags[1 .. 3] are reserved.
 *   The colour by mode: 0 the argument rgb; 1 attr = labels i64[n] through lut u32[n_lut], n_lut >= 3: label < 0 -> lut[0], 0 -> lut[1],
 *   else lut[2 + (label - 1) mod (n_lut - 2)]; 2 attr = values f32 or f64 by attr_f64 through lut u32[256] with lo < hi, both finite:
 *   a NaN value -> nan_rgb, else lut[floor((v - lo) / (hi - lo) * 255 + 0.5) clamped to 0 .. 255]; 3 attr = rgb u8[n, 3].  Only the low
 *   24 bits of a lut entry are used.  A row whose whole footprint is outside its viewport does not read its attribute.
 * tl_raster_keys: grid f64[ny, nx] with grid row 0 the lowest y, an integer zoom >= 1, placed at pixel (x0, y0); the block of ny * zoom
 *   x nx * zoom pixels must lie inside the canvas.  Pixel (py, px) of the block reads cell (ny - 1 - py / zoom, px / zoom): NaN -> key 0,
 *   else the image of float32(value + 0.0) << 32 | the mode-2 colour.  Plain stores: the block is overwritten.
 * tl_render_shade: out u8[height, width, 3]; depth f32[height, width] or null.  A pixel with key 0 gets `background` (depth NaN).  Any
 *   other: d_c = its decoded depth as f64; the neighbours at (dy, dx) in {-radius, 0, radius}^2 without the centre, in row-major order,
 *   contribute d_n - d_c where that is > 0, and 0 where it is not or the neighbour is outside the image or empty; o = their sum in that
 *   order / 8.0; shade = 1.0 / (1.0 + strength * o); a channel is floor(ch * shade + 0.5) (clamped to 0 .. 255, NaN -> 0).
 * A null or misaligned pointer, width or height outside 1 .. 16384, n < 0, ld < 3, n_views outside 1 .. 2^20, mode outside 0 .. 3, size
 * outside 1 .. 9, an rgb beyond 24 bits, n_lut < 3 (mode 1) or != 256 (mode 2), lo >= hi or not finite, a missing attr or lut for the
 * mode, zoom < 1, a raster block outside the canvas, radius outside 1 .. 16, a strength below 0 or not finite, out or depth aliasing
 * keys: TL_ERR_ARG, nothing launched.  Then n = 0 or an empty grid: TL_OK without a kernel launch. */
int tl_splat(const void* pts, int dtype_f64, int64_t ld, int64_t n, const int32_t* vid, const double* views, int n_views, int mode, uint32_t rgb,
             const void* attr, int attr_f64, const uint32_t* lut, int n_lut, double lo, double hi, uint32_t nan_rgb, int size, uint64_t* keys,
             int width, int height, int32_t* flags, tl_stream_t stream);
int tl_raster_keys(const double* grid, int nx, int ny, int zoom, int x0, int y0, const uint32_t* lut, double lo, double hi, uint64_t* keys,
                   int width, int height, tl_stream_t stream);
int tl_render_shade(const uint64_t* keys, int width, int height, int radius, double strength, uint32_t background, uint8_t* out, float* depth,
                    tl_stream_t stream);

/* ------------------------------------------------------------------ LAS point records (csrc/tl_las.hip)
 * The record passes of the LAS reader and writer (treelearn_amd/util/las.py parses and writes the headers on the host).  The layout is
 * the ASPRS one and the rules are restated in numpy in tests/las_restatement.py; all arithmetic is f64 in plain operators, no fma
 * contraction.
 * tl_las_decode: records u8[n * record_length] (device, base aligned to 16), little endian, i32 X Y Z at bytes 0, 4, 8.  Writes rows
 *   first_row .. first_row + n - 1 of out f64[*, out_cols]: x = X * scale[0] + offset[0] (a multiply, then an add), the same for y, z.
 *   out_cols = 4 needs a treeID dimension (tree_id_offset = its byte offset in the record, tree_id_type = 1 .. 10 as the extra-bytes
 *   VLR numbers them: u8 i8 u16 i16 u32 i32 u64 i64 f32 f64) and the classification (the byte at class_offset, and-ed with class_mask:
 *   15 / 0x1f for point formats 0-5, 16 / 0xff for 6-10).  With t = treeID widened to f64 and c the class: label = 0 where c is 1 or
 *   2, else t where t != 0, else -1.  out_cols = 3 takes tree_id_type = 0 and ignores the other three.  `path`: 0 = the library's
 *   choice, 1 = plain (one lane per record, byte loads), 2 = staged (256 records through LDS with 16-byte loads; TL_ERR_UNSUPPORTED
 *   for a record longer than 128 bytes).  Both give the same bits.
 * tl_las_encode: coords f32 or f64 by dtype_f64, n_src rows of stride ld >= 3 elements, labels i64[n_src]; output row j takes source
 *   row order[j] (i64[n]; NULL: j, and n = n_src).  records u8[n * 38] (base aligned to 16): point format 3 + u32 treeID, X =
 *   rint((x - offset) / scale) (subtract, divide, round half to even), intensity 0, return byte 0x09, classification 2 for label 0 and
 *   4 otherwise, scan angle / user data / source 0, GPS time 0.0, RGB = 257 * the three low bytes of h (black for label 0), where
 *   h = (u32)label * 2654435761, h ^= h >> 15, h *= 2246822519, h ^= h >> 13 (mod 2^32), treeID = the low 32 bits of the label.
 *   A row whose coordinate is not finite, whose rint leaves [-2^31, 2^31 - 1] or whose order entry is outside 0 .. n_src - 1 gets an
 *   all-zero record and sets *err (device, 0 otherwise): the caller raises and writes no file.  extremes i32[n_seg, 6] = min X, min Y,
 *   min Z, max X, max Y, max Z of the written rows of each segment (integer atomics: exact for any order; INT32_MAX x 3, INT32_MIN x 3
 *   for a segment without one).  seg_start i64[n_seg + 1] ascending with seg_start[0] = 0 and seg_start[n_seg] = n: segment s holds
 *   output rows seg_start[s] .. seg_start[s + 1] - 1; NULL with n_seg = 1: the whole cloud.
 * A null or misaligned pointer, a negative size, record_length outside 20 .. 65535, a field outside the record, out_cols other than 3
 * or 4, a scale that is not positive and finite (encode), an unknown path: TL_ERR_ARG, nothing launched.  n = 0: TL_OK (encode still
 * resets err and extremes). */
int tl_las_decode(const uint8_t* records, int64_t n, int32_t record_length, int32_t class_offset, int32_t class_mask, int32_t tree_id_offset,
                  int32_t tree_id_type, const double scale[3], const double offset[3], double* out, int32_t out_cols, int64_t first_row,
                  int32_t path, tl_stream_t stream);
int tl_las_encode(const void* coords, int dtype_f64, int64_t ld, int64_t n_src, const int64_t* labels, const int64_t* order, int64_t n,
                  const double scale[3], const double offset[3], const int64_t* seg_start, int64_t n_seg, uint8_t* records, int32_t* err,
                  int32_t* extremes, tl_stream_t stream);

/* ------------------------------------------------------------------ validation metrics of a training run (csrc/tl_train_eval.hip)
 * Replaces `pointwise_eval` (tools/training/train.py:89-102) and the per-tile lists `validate` (:61-86) concatenates for it: called once
 * per validation tile, it ADDS that tile's share to a running state and keeps nothing per point.
 *   logits [n,2], offsets [n,3]: f32 / bf16 / f16 by `dtype` (TL_F32 / TL_BF16 / TL_F16), widened to fp32 on load (the reference's .float());
 *   semantic_labels i64[n]; offset_labels f32[n,3]; mask u8[n] (rows with mask != 0 count; NULL = every row): `masks_sem` of the tile.
 *   Per counted row, in fp32: pred = softmax(logits)[0] >= 0.5 (tree class 0, ties count as tree), tree = semantic_labels == 0;
 *   tp / fp / tn / fn as get_eval_components defines them; for tree rows sum_off += (double) sqrt(sum((offset - offset_label)^2)), n_off += 1
 *   (masks_off = semantic_labels == TREE_CLASS and nothing else, train.py:92).
 *   state: 64 bytes, 8-byte aligned = int64 tp, fp, tn, fn, n_off; float64 sum_off; two reserved words.  Zeroed by the caller before the
 *   first tile, read back once after the last: acc = (tp + tn) / (tp + fp + tn + fn), Offset_MAE = sum_off / n_off.
 *   ws: tl_pointwise_eval_ws_bytes(n) bytes of per-workgroup partials.  Two stages (workgroup partials, then one workgroup that sums them
 *   in index order), integer counts and a float64 sum, no float atomics: the state is bit-reproducible from run to run.
 *   n = 0 is a no-op.  Arrays that are 16-byte aligned are read with 16-byte loads, four rows per lane; any other alignment of whole
 *   elements is served row by row. */
int64_t tl_pointwise_eval_ws_bytes(int64_t n);
int tl_pointwise_eval(const void* logits, const void* offsets, int dtype, const int64_t* semantic_labels, const float* offset_labels,
                      const uint8_t* mask, int64_t n, void* state, void* ws, tl_stream_t stream);

/* ------------------------------------------------------------------ training / validation batches on the device (csrc/tl_train_batch.hip)
 * Replaces the per-item numpy work of TreeDataset.__getitem__ (tree_learn/dataset/dataset.py:34-140) and the concatenation of
 * collate_fn (:167-226) for crops and tiles whose rows are already in HBM.
 *
 * tl_point_jitter <- point_jitter (dataset.py:92-95), in place on xyz f32[n,3]: x <- f32(f64(x) + clip(0.1 g, -0.2, 0.2)).  g is a standard
 *   normal from a counter-based generator (splitmix64 of (key, row, component) -> two uniforms -> Box-Muller in f64): a function of
 *   (key, row, component) only, so the same key gives the same bits for any launch shape.  These are NOT numpy's draws: a run that
 *   jitters is statistically, not bitwise, the reference's.
 *
 * tl_train_item <- dataset.py:41-66 (labels, centre, masks), :85-89 (the matrix of transform_train), :111-140 (offset labels), fused; ONE crop
 *   or tile per call, written at rows [row_offset, row_offset + n) of batch-sized outputs, so collate_fn's concatenation is the offset.
 *   xyz f32[n,3], instance_label i32[n] (device); m = HOST f64[9], row-major, or NULL for test mode; center = HOST f32[3], or NULL for the
 *   training dummy of ones.  Outputs (device, batch bases): coords f32[.,3], semantic_labels i64 (label 0 -> 1, else 0), instance_labels
 *   i64, offset_labels f32[.,3], masks_inner / masks_off / masks_sem u8, batch_ids i64 (= batch_id), centers f32[.,3].  Features are not
 *   touched: they stay a plain copy.
 *   Coordinate type: with m, c = x m[0][k] + y m[1][k] + z m[2][k] in f64 (no fma contraction), coords = f32(c), and every comparison and
 *   the offset subtraction are f64 on c (np.matmul(xyz32, m64) makes the reference's training items float64); without m they are f32 on
 *   the stored values and `low + 0.5` is rounded to f32 (the reference's test items stay float32).
 *   Tree base, per distinct label != 0 (any int32 values, any number of them; -1 is an instance of its own here, masks_off removes it):
 *   low = the 4th smallest z, RANK 3 WITH DUPLICATES COUNTED (np.sort(z)[3]), for an instance of more than 11 rows, its minimum otherwise.
 *   The reference's np.partition(z, 10)[3] is an implementation-defined element among the ten lowest; the device rule is rank 3 by
 *   definition.  position = f32(mean of the instance's rows with z <= low + 0.5); the sum is an exact INTEGER sum: every addend is
 *   floor(c * 2^60) as a 128-bit two's-complement integer (split as trunc(c) + the exact remainder; off by less than 2^-60 per addend, for
 *   every finite c including -0.0 and tiny negatives), added with integer atomics; coordinates must be finite and below 2^32 in magnitude.
 *   The division is f64.  offset = f32(position - c); rows of label 0 get
 *   position = 1.  masks_inner = max(|x|, |y|) <= half_inner; masks_sem = inner & (label != -1); masks_off = masks_sem & (label != 0)
 *   (the reference's `valid` is always true for a tree instance: the row of rank 3 is a base row).
 *   No floating-point atomics: two calls on the same input give identical bits, at any row_offset.
 *   ws: tl_train_item_ws_bytes(n) bytes, 256-byte aligned (label table, per-row slot and z image, 128 B per possible instance).
 *   n <= 0, n > 2^30, a null or misaligned pointer: TL_ERR_ARG, nothing launched (tl_train_item_ws_bytes returns 0 for such n). */
int tl_point_jitter(float* xyz, int64_t n, uint64_t key, tl_stream_t stream);
int64_t tl_train_item_ws_bytes(int64_t n);
int tl_train_item(const float* xyz, const int32_t* instance_label, int64_t n, const double* m, double half_inner, const float* center,
                  int64_t batch_id, int64_t row_offset, float* coords, int64_t* semantic_labels, int64_t* instance_labels,
                  float* offset_labels, uint8_t* masks_inner, uint8_t* masks_off, uint8_t* masks_sem, int64_t* batch_ids, float* centers,
                  void* ws, tl_stream_t stream);

/* ------------------------------------------------------------------ points against the plot outline (csrc/tl_hull.hip)
 * Replaces `get_coords_within_shape` (tree_learn/util/pipeline.py:211-223: a shapely Point per point + a geopandas sjoin) on the
 * polygon of `get_hull` (:256-265) and on the ring buffer of `get_hull_buffer` (:240-253), as tools/pipeline/pipeline.py:80-81,136-142,
 * 168-169 call it.  The ring is f64[V,2], CLOSED (first vertex repeated last): segments (x1,y1) = ring[k], (x2,y2) = ring[k+1], k < V-1.
 * Per point (x = row[0], y = row[1] of pts, f32 or f64, row stride ld elements), in f64, plain operators, no fma contraction:
 *   bit 0 (strictly inside, even-odd): parity over segments of [(y1 > py) != (y2 > py) and px < x1 + (py - y1) * (x2 - x1) / (y2 - y1)];
 *   bit 1 (distance < r): any segment with t = ((px-x1)*dx + (py-y1)*dy) / (dx*dx + dy*dy) clamped to [0, 1], qx = x1 + t*dx,
 *     qy = y1 + t*dy, (px-qx)*(px-qx) + (py-qy)*(py-qy) < r*r  (dx = x2-x1, dy = y2-y1); never set when r = 0.
 * Both bits equal that formula evaluated over every segment (numpy); the per-point work reads only the point's slab and cell lists.
 * The grid struct below is host-filled: slabs of height slab_h from slab_lo cover the ring's y-range widened by pad; cells (nx x ny, edge h, from lo)
 * cover the ring's box widened by r + pad, nx = ny = 0 when r = 0; pad = the rounding allowance of the pruning; cover_r2 = (r - 2 pad)^2,
 * or 0 to skip the covered-cell shortcut.
 * tl_ring_lists: count pass (cell_seg = slab_seg = NULL): cell_cnt i64[nx*ny], slab_cnt i64[nslab] ZEROED by the caller, incremented per
 *   listed segment; fill pass: the same arrays holding the exclusive starts on entry (advanced as cursors), lists i32 written at them.
 *   Order within a list is not deterministic and does not affect any bit.
 * tl_ring_covered: covered u8[nx*ny] = 1 if the whole cell is within sqrt(cover_r2) of one listed segment (cell_start i64[nx*ny + 1]).
 * tl_ring_classify: out u8[n]; slab_start i64[nslab + 1]. */
typedef struct {
  double lo[2], h, r, pad, cover_r2, slab_lo, slab_h;
  int32_t nx, ny, nslab, reserved;
} tl_ring_grid;
int tl_ring_lists(const double* ring, int64_t V, const tl_ring_grid* grid, int64_t* cell_cnt, int64_t* slab_cnt, int32_t* cell_seg,
                  int32_t* slab_seg, tl_stream_t stream);
int tl_ring_covered(const double* ring, const tl_ring_grid* grid, const int64_t* cell_start, const int32_t* cell_seg, uint8_t* covered,
                    tl_stream_t stream);
int tl_ring_classify(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* ring, const tl_ring_grid* grid,
                     const int64_t* slab_start, const int32_t* slab_seg, const int64_t* cell_start, const int32_t* cell_seg,
                     const uint8_t* covered, uint8_t* out, tl_stream_t stream);


/* ------------------------------------------------------------------ the whole eval-mode forward behind ONE call
 * Replaces, per batch of tiles, the body of `model(batch, return_loss=False)` of the reference's tile loop
 * (tree_learn/util/pipeline.py:86 -> tree_learn/model/tree_learn.py:75-103: voxelize :129-167, input conv :90, UBlock recursion
 * blocks.py:137-149, output_layer :93, forward_head :97-103): the yaml's configuration (use_feats = use_coords = False: all-ones
 * voxel features, configs/_modular/model.yaml:5-6) and the constructor's own defaults (use_feats = True, tree_learn.py:18: voxel-mean
 * features, tl_voxel_feats).  tl_forward enqueues everything the per-operator entry points
 * above would be called for -- tl_voxel_point_coords, tl_pyramid_build, tl_blk_build, tl_rulebooks_build, every tl_conv_fwd of the
 * U-Net in the pre-activated dataflow (BatchNorm + ReLU folded into producer epilogues / the staging prologue, residual adds and the
 * skip concat as views) and tl_head_mlp -- from C, so that the host cost of a forward no longer depends on the caller's interpreter.
 * It SYNCHRONISES `stream` twice (grid extent, level counts: two 16-B read-backs, as the per-operator path does).
 *
 * The network is described by plain structs of DEVICE pointers the caller keeps alive (weights in the tl_pack_weight layout, `frag` =
 * the tl_pack_weight_frag copy or NULL, eval-mode BatchNorms as scale / shift); nothing is copied.  All device memory of one forward
 * -- geometry and activations -- comes out of ONE caller-provided arena; if it is too small the call returns TL_ERR_ARENA with
 * args->needed_bytes set and nothing useful enqueued (call again with a larger arena).  Outputs are caller-provided and never alias
 * the arena, so the arena may serve the next forward on the same stream at once. */
#define TL_MAX_LEVELS 8
#define TL_ERR_ARENA (-4)        /* arena too small: args->needed_bytes */
#define TL_ERR_REACH_ZERO (-5)   /* a level's spatial shape or voxel set collapsed (spconv's "reach zero!!!", util/pipeline.py:91-97) */
#define TL_ERR_BLK (-7)          /* the block-local unit builder flagged skipped units (an internal assertion: cannot happen with the capacities tl_forward
                                    passes).  The flag comes home BEHIND the forward that raised it: tl_exec_check reports it for the forwards enqueued so
                                    far; a tl_forward that finds it set by its predecessor on the context returns it before enqueuing anything */
#define TL_ERR_EXTENT (-6)       /* the tile's voxel extent exceeds spatial_shape, a batch id is out of range, or a voxel coordinate leaves [0, 65536) */
typedef struct tl_affine { const float* scale; const float* shift; } tl_affine;
typedef struct tl_weight { const void* w; const void* frag; int32_t K, Cout, Cin, reserved; const void* x3; /* tl_pack_weight_x3 copy or NULL */ } tl_weight;
typedef struct tl_res_desc {      /* ResidualBlock, blocks.py:42-79 */
  tl_affine bn0; tl_weight w1; tl_affine bn3; tl_weight w2;
  tl_weight w1x1;                 /* i_branch: w == NULL = Identity (blocks.py:48-52) */
  tl_weight w1_half[2];           /* w1 split into its two input-channel halves (2C -> C decoder block on block-local rows), w == NULL = absent */
} tl_res_desc;
typedef struct tl_ublock_desc {   /* UBlock, blocks.py:81-149 (block_reps = 2, tree_learn.py:41) */
  int32_t C; int32_t deeper;
  tl_res_desc blocks[2];
  tl_affine bn_down; tl_weight wd;      /* BN, ReLU, SparseConv3d k2 s2 (blocks.py:102-110) */
  tl_affine bn_up; tl_weight wu;        /* BN, ReLU, SparseInverseConv3d k2 (blocks.py:116-123) */
  tl_res_desc tail[2];
  tl_affine bn_cat_l, bn_cat_r;         /* tail[0].bn0 split over the two halves of the skip concat (blocks.py:146) */
} tl_ublock_desc;
typedef struct tl_net_desc {
  int32_t dtype;                  /* TL_F32 | TL_BF16 | TL_F16 */
  int32_t num_levels;             /* 2 .. TL_MAX_LEVELS */
  float voxel_size;
  int32_t has_shape; int32_t spatial_shape[3];   /* tree_learn.py:86-87 override; has_shape = 0: the tile's own extent (:165) */
  int32_t blocked;                /* != 0: level 1 may run in the block-local order (16-bit, C = 32) */
  int32_t in_channels;            /* dim_coord + dim_feat of the input conv (tree_learn.py:38) */
  int32_t use_coords, use_feats;  /* tree_learn.py:152-155: both 0 = all-ones voxel features (no gather in the input conv); else args->point_feats is read */
  int32_t max_points_per_voxel;   /* tree_learn.py:22,141 (read when use_coords | use_feats) */
  int32_t reserved0;
  tl_weight w_in;                 /* input conv, tree_learn.py:37-39 */
  tl_ublock_desc u[TL_MAX_LEVELS];
  tl_affine out_bn;               /* output_layer, tree_learn.py:42 */
  const float* head_w1; const float* head_b1; const float* head_w2; const float* head_b2;   /* as tl_head_mlp takes them */
} tl_net_desc;
typedef struct tl_launch_rec {    /* one conv launch of a profiled forward */
  int32_t level, kind;            /* kind: 0 = SubM (27 taps), 1 = stride-2, 2 = inverse, 3 = 1x1, 4 = input conv */
  int32_t K, Cin, Cout, residual, esize, split_part, split_cin, in_prologue;
  int64_t n_out, n_in;
  float ms;
} tl_launch_rec;
typedef struct tl_forward_args {
  const float* xyz; const int64_t* batch_ids; int64_t N; int32_t B; int32_t reserved;
  const float* point_feats;       /* f32[N, in_channels - 3] (batch['input_feats']); may be NULL when the net uses neither coordinates nor features */
  void* arena; int64_t arena_bytes;
  float* backbone;                /* f32[N, C] or NULL */
  float* logits; float* offsets;  /* f32[N, 2], f32[N, 3] */
  tl_stream_t side_stream;        /* optional: the block-local unit builder runs there beside the other levels' rulebook kernels */
  int64_t needed_bytes;           /* out */
  int64_t level_n[TL_MAX_LEVELS]; /* out: active voxels per level */
  int32_t blocked_used;           /* out */
  int32_t launches;               /* out: tl_conv_fwd launches enqueued */
} tl_forward_args;
typedef struct tl_exec tl_exec;   /* host-side context of a caller thread / stream: pinned read-back words, two events, profile storage */
tl_exec* tl_exec_create(void);
void tl_exec_destroy(tl_exec* ex);
int tl_forward(tl_exec* ex, const tl_net_desc* net, tl_forward_args* args, tl_stream_t stream);
/* Waits for the unit-builder flag of the LAST tl_forward enqueued on this context (a 4-byte read-back behind its geometry kernels, not
 * behind its convs) and returns TL_ERR_BLK if that forward or an unreported earlier one raised it, else TL_OK.  Callers that need the
 * verdict for a particular tile call it before the next tl_forward on the context; a tile loop calls it once after its last tile. */
int tl_exec_check(tl_exec* ex);
/* Live per-launch timing of the NEXT tl_forward calls on this context (HIP events on the launch stream around every conv launch;
 * enable = 0 stops).  tl_exec_profile_read waits for the last profiled forward and returns its launches (<= cap; return value = their
 * number, negative = error). */
int tl_exec_profile(tl_exec* ex, int enable);
int tl_exec_profile_read(tl_exec* ex, tl_launch_rec* recs, int cap);


#ifdef __cplusplus
}
#endif
#endif /* TREELEARN_HIP_H */
