// Sparse convolution forward (SubMConv3d / SparseConv3d / SparseInverseConv3d / 1x1) for gfx950: the dispatch.
//
// tl_conv_fwd = validate -> fill ConvP -> walk an ordered list of rungs, each "guard, then try one kernel family" ("Conv
// dispatch").  The kernels live in the family units (tl_conv_*.hip, tl_linear_small.hip); every one of them launches through tl_launch
// (tl_common.h), so tl_conv_route can run this very code with the launches replaced by records.  This unit also owns the developer
// switches (tl_set_tuning) the rungs consult.
#include "tl_conv_internal.h"
#include <cxxabi.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// ---- route mode (tl_common.h: tl_launch).  One record per launch the armed thread would have made, joined by " + ".
struct TlRoute {
  char text[1024] = "";
  int len = 0;
  bool truncated = false;
};
thread_local TlRoute* tl_route_armed = nullptr;

// `tag` demangles to "TlKernelTag<&(void (anonymous namespace)::k_name<args>(ConvP, ...))>" -> "k_name<args>"
int tl_route_record(TlRoute* r, const char* tag, bool f16, dim3 grid, dim3 block, size_t lds) {
  int status = 0;
  char* full = abi::__cxa_demangle(tag, nullptr, nullptr, &status);
  struct Free { char* p; ~Free() { free(p); } } guard{full};
  const char* b = (status == 0 && full) ? strstr(full, "&(") : nullptr;
  b = b ? b + 2 : tag;
  const char* e = b;
  for (int depth = 0; *e; ++e) {                  // the identifier in front of the first '<' or '(' that is not the anonymous namespace's
    if (!strncmp(e, "(anonymous namespace)", 21)) { e += 20; continue; }
    if (depth == 0 && (*e == ' ' || *e == ':')) b = e + 1;
    if (depth == 0 && *e == '(') break;
    depth += (*e == '<') - (*e == '>');
    if (depth == 0 && *e == '>') { ++e; break; }
  }
  char dims[2][40];
  const dim3 d[2] = {grid, block};
  for (int i = 0; i < 2; ++i) {
    if (d[i].y == 1 && d[i].z == 1) snprintf(dims[i], sizeof dims[i], "%u", d[i].x);
    else snprintf(dims[i], sizeof dims[i], "(%u, %u, %u)", d[i].x, d[i].y, d[i].z);
  }
  const int room = (int)sizeof r->text - r->len;
  const int n = snprintf(r->text + r->len, (size_t)room, "%s%.*s%s<<<%s, %s, %zu>>>", r->len ? " + " : "", (int)(e - b), b, f16 ? "/f16" : "", dims[0], dims[1], lds);
  if (n < 0 || n >= room) { r->truncated = true; r->text[r->len] = 0; return TL_OK; }
  r->len += n;
  return TL_OK;
}

// ---- developer switches (tl_set_tuning)
static int64_t g_small_rows = 16384;              // below this the 128-row tilings cannot fill 256 CUs: the small-level kernel (tl_conv_small.hip)
extern int g_small_mode;                          // tl_conv_small.hip
extern int g_wgrad_dense;                         // tl_wgrad_dense.hip
extern int64_t g_wgrad_dense_min_rows;
extern int g_wgrad_rows;                          // tl_wgrad_rows.hip
extern int g_wgrad_dma;                           // tl_wgrad_dense.hip
static int g_stream = 1;                          // use the streamed-weights register-gather kernel where it applies
static int g_streamq = 1;                         // ... and its quad-gather form for bf16 with Cin % 64 == 0
static int g_streamq_x3 = 1;                      // ... and for fp32 rows in the parity-fast mode (tl_set_tuning "streamq_x3")
static int g_direct = 1;                          // use the weights-in-LDS direct kernel where it applies
static int g_direct_oh = 1;                       // ... and its gather-once form for the level-1 inverse conv
static int g_blk = 1;                             // use the staged-unit kernel when the caller passes the block-local rulebook form
static int g_up = 1;                              // use the coarse-stationary inverse conv when the caller passes the scatter form of the table

// (tl_exec.hip: may the forward hand the level-1 inverse conv its packed table?  Developer switches can take the gather-once kernel away.)
bool tl_conv_one_hot_direct_enabled(int64_t n_out) { return g_direct && g_direct_oh && n_out > g_small_rows; }     // (small levels: the small-level kernel serves the conv, from the [8][n] table)

namespace {

// ---- the alignment facts of one call, each computed ONCE.  Different moduli are different fields: the 16-bit kernels move rows as 8-element
// vectors, the fp32 ones as 4-element vectors; the staged-unit kernel reads the affine through scalar loads (4 B), the others as 16-B vectors.
struct ConvAlign {
  bool in16, in8;                 // `in` 16-B / 8-B aligned
  bool w16, w4;                   // `weight` 16-B / 4-B aligned
  bool in_ld8, in_ld4;            // input row stride a multiple of 8 / 4 elements
  bool out_vec;                   // every given view: 16-B aligned, row stride a multiple of 8 elements
  bool in_aff16;                  // gather-side affine absent or 16-B aligned
  bool out_aff16, out_aff4;       // first view's affine absent or 16-B / 4-B aligned
  bool res_ld8, res_ld4;          // residual absent or 16-B aligned with a row stride that is a multiple of 8 / 4 elements
  bool vec_ok() const { return in_ld8 && in16 && w16; }                        // input rows and weights as 8-element vectors
  bool aligned() const { return in_ld4 && in16 && w16 && in_aff16; }           // ... as 4-element vectors, with the prologue's affine
};

bool ptr_al(const void* p, unsigned bytes) { return ((uintptr_t)p) % bytes == 0; }

ConvAlign conv_align(const tl_conv_args* a) {
  ConvAlign c;
  c.in16 = ptr_al(a->in, 16); c.in8 = ptr_al(a->in, 8);
  c.w16 = ptr_al(a->weight, 16); c.w4 = ptr_al(a->weight, 4);
  c.in_ld8 = a->in_ld % 8 == 0; c.in_ld4 = a->in_ld % 4 == 0;
  c.out_vec = a->out_ld % 8 == 0 && ptr_al(a->out, 16) && (!a->out2 || (a->out2_ld % 8 == 0 && ptr_al(a->out2, 16))) && (!a->out3 || (a->out3_ld % 8 == 0 && ptr_al(a->out3, 16)));
  c.in_aff16 = !a->in_scale || (ptr_al(a->in_scale, 16) && ptr_al(a->in_shift, 16));
  c.out_aff16 = !a->out_scale || (ptr_al(a->out_scale, 16) && ptr_al(a->out_shift, 16));
  c.out_aff4 = !a->out_scale || (ptr_al(a->out_scale, 4) && ptr_al(a->out_shift, 4));
  c.res_ld8 = !a->residual || (a->res_ld % 8 == 0 && ptr_al(a->residual, 16));
  c.res_ld4 = !a->residual || (a->res_ld % 4 == 0 && ptr_al(a->residual, 16));
  return c;
}

// ---- one call on its way down the ladder
struct Conv {
  const tl_conv_args* a;
  ConvP p;
  ConvAlign al;
  const TlConvH16* L;             // the launchers of this call's 16-bit type (tl_conv_internal.h)
  int dt;                         // TL_F32 | TL_BF16 = "the 16-bit type": what the launchers are told
  bool f16, train, has_blk;
  hipStream_t s;
  bool mult32() const { return a->Cin % 32 == 0 && a->Cout % 32 == 0; }
  bool no_prologue() const { return !a->in_scale && !a->in_relu; }
};

// a rung returns TL_NEXT to pass the call on to the next rung, anything else ends the dispatch
constexpr int TL_NEXT = 1;
int or_next(int rc) { return rc == TL_ERR_UNSUPPORTED ? TL_NEXT : rc; }         // "this family has no kernel for the shape" is not an answer yet

int validate(const tl_conv_args* a, bool has_blk) {
  if (!a->table && a->K != 1 && !has_blk && !(a->in_all_ones && a->blk_pmask)) return TL_ERR_ARG;
  if ((a->in_scale == nullptr) != (a->in_shift == nullptr)) return TL_ERR_ARG;
  if ((a->out_scale == nullptr) != (a->out_shift == nullptr)) return TL_ERR_ARG;
  if (a->dtype != TL_F32 && a->dtype != TL_BF16 && a->dtype != TL_F16) return TL_ERR_ARG;
  if ((a->out2_scale == nullptr) != (a->out2_shift == nullptr) || (a->out3_scale == nullptr) != (a->out3_shift == nullptr)) return TL_ERR_ARG;
  if (a->epi_mode != TL_EPI_NONE) {                             // only the direct / stream / staged-unit families carry the training epilogues
    if ((a->epi_mode != TL_EPI_STATS && a->epi_mode != TL_EPI_BN_BWD) || !a->red_part || ((uintptr_t)a->red_part) % 8) return TL_ERR_ARG;
    if (a->epi_mode == TL_EPI_BN_BWD) {
      if (!a->bn_x || !a->bn_mean || !a->bn_rstd || !a->bn_scale || !a->bn_shift) return TL_ERR_ARG;
      if (a->bn_x_ld % 8 || !ptr_al(a->bn_x, 16) || !ptr_al(a->bn_mean, 16) || !ptr_al(a->bn_rstd, 16) || !ptr_al(a->bn_scale, 16) || !ptr_al(a->bn_shift, 16)) return TL_ERR_UNSUPPORTED;
    }
  }
  return TL_OK;
}

ConvP fill_convp(const tl_conv_args* a, bool has_blk) {
  ConvP p;
  p.in = a->in; p.in_ld = a->in_ld; p.w = a->weight; p.w_frag = a->weight_frag;
  p.w_x3 = (a->dtype == TL_F32 && a->Cin % 32 == 0 && ptr_al(a->weight_x3, 16)) ? a->weight_x3 : nullptr;
  p.table = a->table; p.ctab = (a->K == 27) ? a->table_compact : nullptr; p.n_out = a->n_out; p.n_in = a->n_in;
  p.K = a->K; p.Cin = a->Cin; p.Cout = a->Cout; p.in_scale = a->in_scale; p.in_shift = a->in_shift;
  p.in_relu = a->in_relu; p.out_relu = a->out_relu; p.res = a->residual; p.res_ld = a->res_ld;
  p.out_scale = a->out_scale; p.out_shift = a->out_shift; p.out = a->out; p.out_ld = a->out_ld;
  p.out2 = a->out2; p.out2_ld = a->out2_ld; p.out2_scale = a->out2_scale; p.out2_shift = a->out2_shift; p.out2_relu = a->out2_relu;
  p.out3 = a->out3; p.out3_ld = a->out3_ld; p.out3_scale = a->out3_scale; p.out3_shift = a->out3_shift; p.out3_relu = a->out3_relu;
  p.nblk = (int)tl_cdiv(a->n_out, TL_CONV_TILE_ROWS);
  p.one_hot = a->table != nullptr ? a->table_one_hot : 0;
  p.blk_unit = has_blk ? a->blk_unit : nullptr; p.blk_counter = a->blk_counter; p.blk_halo = a->blk_halo; p.blk_lrb = a->blk_lrb;
  p.blk_pmask = a->K == 27 ? a->blk_pmask : nullptr;
  p.epi_mode = a->epi_mode; p.red_part = a->red_part; p.red_nparts = a->red_nparts; p.bn_x = a->bn_x; p.bn_x_ld = a->bn_x_ld;
  p.bn_mean = a->bn_mean; p.bn_rstd = a->bn_rstd; p.bn_scale = a->bn_scale; p.bn_shift = a->bn_shift; p.bn_relu = a->bn_relu;
  return p;
}

// ------------------------------------------------------------------------------------------------------------------ the rungs, in order
// packed one-hot table (tl_level.inv_packed): only the gather-once form of the direct kernel decodes it (16-bit, or fp32 rows with split-bf16
// weights; 8 taps, 64 -> 32) -- everything else would read it as an [8][n] table
int rung_packed_one_hot(Conv& c) {
  if (c.p.one_hot != 2) return TL_NEXT;
  const tl_conv_args* a = c.a;
  const bool shape = a->K == 8 && a->Cin == 64 && a->Cout == 32 && !c.train && c.no_prologue() && g_direct && g_direct_oh;
  if (!shape || !(c.dt == TL_BF16 || (c.dt == TL_F32 && c.p.w_x3))) return TL_ERR_UNSUPPORTED;
  return c.L->direct(c.p, c.dt, c.s);
}

// all-ones input: presence masks instead of a gather
int rung_ones27(Conv& c) {
  const tl_conv_args* a = c.a;
  if (!(a->in_all_ones && !c.train && c.al.out_vec && (g_direct || !a->table) && c.al.w4 && !a->residual)) return TL_NEXT;
  return or_next(c.L->ones27(c.p, c.dt, c.s));
}

// block-local rows, 16-bit: the staged-unit kernel
int rung_blk(Conv& c) {
  const tl_conv_args* a = c.a;
  if (!(c.has_blk && c.dt == TL_BF16 && g_blk && c.al.vec_ok() && c.al.out_vec && c.al.res_ld8 && c.al.out_aff4 && (!a->in_relu || a->in_scale))) return TL_NEXT;
  return or_next(c.L->blk(c.p, c.s));
}

// bf16x3 on block-local rows: the staged-unit kernel for fp32 rows (two launches)
int rung_blk_x3(Conv& c) {
  if (!(c.has_blk && c.a->dtype == TL_F32 && c.p.w_x3 && g_blk && !c.train)) return TL_NEXT;
  return or_next(tl_launch_conv_blk_x3(c.p, c.s));
}

// block-local rows without a shape the staged-unit kernels serve, and no plain table to fall back on
int rung_needs_table(Conv& c) { return (!c.a->table && c.a->K != 1) ? TL_ERR_UNSUPPORTED : TL_NEXT; }

// inverse conv walking the coarse rows (levels 1-4)
int rung_up(Conv& c) {
  const tl_conv_args* a = c.a;
  if (!(a->table_scatter && c.p.one_hot && g_up && !c.train && c.dt == TL_BF16 && c.al.vec_ok() && c.al.out_vec && c.al.out_aff16)) return TL_NEXT;
  return or_next(c.L->up(c.p, a->table_scatter, c.s));
}

// the 4-channel input conv, 16-bit (8-B rows)
int rung_in4(Conv& c) {
  const tl_conv_args* a = c.a;
  if (!(c.dt == TL_BF16 && a->Cin == 4 && a->Cout == 32 && g_direct && c.al.out_vec && c.al.in8 && c.al.w16 && c.al.res_ld8)) return TL_NEXT;
  return or_next(c.L->direct(c.p, TL_BF16, c.s));
}

// at most 8 input channels: the answer, whatever it is
int rung_tinycin(Conv& c) {
  const tl_conv_args* a = c.a;
  if (!(!c.train && a->Cin <= 8 && a->Cout % 8 == 0 && a->Cout <= 64 && c.no_prologue() && c.al.out_vec)) return TL_NEXT;
  return c.L->tinycin(c.p, c.dt, c.s);
}

// small levels: the small-level kernel in inference; in training the separate passes
int rung_small(Conv& c) {
  if (!c.train && c.al.vec_ok() && c.a->n_out <= g_small_rows && c.mult32()) return c.L->small(c.p, c.dt, c.s);
  if (c.train && c.a->n_out <= g_small_rows) return TL_ERR_UNSUPPORTED;
  return TL_NEXT;
}

// split-bf16 weights of a wide conv come as two half-width convs (tl_pack_weight_x3): the decoder's 2C -> C conv of level 4 (256 -> 128)
// runs as two 128 -> 128 launches, the first leaving its raw sums in `out`, the second taking them as its residual.  Whether or not that
// serves the call, the rungs below must not see the half layout: it is not what the single-launch kernels read.
int rung_wide_x3_split(Conv& c) {
  const tl_conv_args* a = c.a;
  if (!(c.p.w_x3 && a->Cin >= 256)) return TL_NEXT;
  const ConvP p = c.p;
  c.p.w_x3 = nullptr;                                            // <- for every later rung
  if (!(c.dt == TL_F32 && !c.train && g_stream && c.al.aligned() && c.al.out_vec && a->Cin % 64 == 0 && a->Cout % 32 == 0 && c.no_prologue() && !a->residual &&
        !a->out2 && !a->out3 && a->n_out > g_small_rows && c.al.out_aff16))
    return TL_NEXT;
  ConvP p1 = p;
  p1.Cin = a->Cin / 2; p1.out_scale = nullptr; p1.out_shift = nullptr; p1.out_relu = 0;
  const int rc1 = c.L->stream(p1, TL_F32, c.s);
  if (rc1 != TL_OK) return or_next(rc1);
  ConvP p2 = p;
  p2.Cin = a->Cin / 2; p2.in = static_cast<const float*>(a->in) + a->Cin / 2;
  p2.w_x3 = static_cast<const char*>(p.w_x3) + (size_t)a->K * a->Cout * (a->Cin / 2) * 4;
  p2.res = a->out; p2.res_ld = a->out_ld;
  return c.L->stream(p2, TL_F32, c.s);
}

// fp32 rows, resident or streamed weights
bool f32_vec(const Conv& c) { return c.dt == TL_F32 && c.al.aligned() && c.al.out_vec && c.mult32() && c.no_prologue() && c.al.res_ld4 && c.al.out_aff16; }
int rung_f32_direct(Conv& c) { return f32_vec(c) && g_direct ? or_next(c.L->direct(c.p, TL_F32, c.s)) : TL_NEXT; }
int rung_f32_streamq_x3(Conv& c) {                               // bf16x3: quad-coalesced gathers where the shape has an instantiation
  if (!(f32_vec(c) && g_stream && g_streamq && g_streamq_x3 && c.p.w_x3 && !c.train && c.a->n_out > g_small_rows)) return TL_NEXT;
  return or_next(tl_launch_conv_streamq_x3(c.p, c.s));
}
int rung_f32_stream(Conv& c) { return f32_vec(c) && g_stream ? or_next(c.L->stream(c.p, TL_F32, c.s)) : TL_NEXT; }

// fp32 below here: no training epilogues
int rung_f32_train_ends(Conv& c) { return (c.train && c.dt == TL_F32) ? TL_ERR_UNSUPPORTED : TL_NEXT; }

// fp32 shapes none of the resident-weight / streamed-weight kernels has an instantiation for (the level-4 <- 5 inverse conv 160 -> 128 on 38 k
// rows): the small-level kernel before the tile kernel while the level is still small (0.198 -> 0.082 ms in the parity-fast mode)
int rung_f32_small(Conv& c) {
  if (!(c.dt == TL_F32 && c.al.vec_ok() && c.a->n_out <= 4 * g_small_rows && c.mult32() && c.no_prologue())) return TL_NEXT;
  return c.L->small(c.p, c.dt, c.s);
}

int rung_f32_tile(Conv& c) {
  if (!(c.dt == TL_F32 && c.al.aligned() && c.mult32() && c.a->Cout <= 224)) return TL_NEXT;
  return tl_launch_conv_mfma_f32(c.p, c.s);
}

// 16-bit rows
bool h16_vec(const Conv& c) {
  return c.dt == TL_BF16 && c.al.aligned() && c.al.vec_ok() && c.al.out_vec && c.mult32() && c.a->Cout <= 224 && c.al.res_ld8 && c.al.out_aff16;
}
int rung_h16_one_hot_direct(Conv& c) {                           // level-1 inverse conv: weights resident, no barriers
  if (!(h16_vec(c) && c.p.one_hot && g_direct && g_direct_oh && c.a->K == 8 && c.a->Cin == 64 && c.a->Cout == 32)) return TL_NEXT;
  return or_next(c.L->direct(c.p, TL_BF16, c.s));
}
int rung_h16_one_hot_stream(Conv& c) {                           // inverse convs: the stream kernel's gather-once form
  return h16_vec(c) && c.p.one_hot && g_stream && c.a->K == 8 ? or_next(c.L->stream(c.p, TL_BF16, c.s)) : TL_NEXT;
}
int rung_h16_direct(Conv& c) { return h16_vec(c) && g_direct ? or_next(c.L->direct(c.p, TL_BF16, c.s)) : TL_NEXT; }
int rung_h16_streamq(Conv& c) { return h16_vec(c) && g_stream && g_streamq ? or_next(c.L->streamq(c.p, c.s)) : TL_NEXT; }
int rung_h16_stream(Conv& c) { return h16_vec(c) && g_stream ? or_next(c.L->stream(c.p, TL_BF16, c.s)) : TL_NEXT; }
int rung_h16_tile(Conv& c) {                                     // the answer for vector-aligned 16-bit rows (no training epilogue)
  if (!h16_vec(c)) return TL_NEXT;
  return c.train ? TL_ERR_UNSUPPORTED : c.L->bf16(c.p, c.s);
}

// scalar fallbacks: TL_F32 / TL_BF16 only, inference only
int rung_scalar_only(Conv& c) { return (c.train || c.f16) ? TL_ERR_UNSUPPORTED : TL_NEXT; }
int rung_tinycout(Conv& c) { return or_next(tl_launch_conv_tinycout(c.p, c.dt, c.s)); }       // 1x1 with <= 8 output channels (the heads' output Linears in training)
int rung_generic(Conv& c) { return tl_launch_conv_generic(c.p, c.dt, c.s); }

// THE ORDER.  Moving a rung sends layers to another family: another speed, other low bits (tests/test_host_conv_route.py pins the routes).
constexpr int (*kLadder[])(Conv&) = {
    rung_packed_one_hot, rung_ones27, rung_blk, rung_blk_x3, rung_needs_table, rung_up, rung_in4, rung_tinycin, rung_small, rung_wide_x3_split,
    rung_f32_direct, rung_f32_streamq_x3, rung_f32_stream, rung_f32_train_ends, rung_f32_small, rung_f32_tile,
    rung_h16_one_hot_direct, rung_h16_one_hot_stream, rung_h16_direct, rung_h16_streamq, rung_h16_stream, rung_h16_tile,
    rung_scalar_only, rung_tinycout, rung_generic,
};

}  // namespace

extern "C" {

int tl_set_tuning(const char* key, int64_t value) {
  if (!key) return TL_ERR_ARG;
  if (!strcmp(key, "direct")) { g_direct = (int)value; return TL_OK; }
  if (!strcmp(key, "blk")) { g_blk = (int)value; return TL_OK; }
  if (!strcmp(key, "up")) { g_up = (int)value; return TL_OK; }
  if (!strcmp(key, "direct_oh")) { g_direct_oh = (int)value; return TL_OK; }
  if (!strcmp(key, "stream")) { g_stream = (int)value; return TL_OK; }
  if (!strcmp(key, "streamq")) { g_streamq = (int)value; return TL_OK; }
  if (!strcmp(key, "streamq_x3")) { if (value != 0 && value != 1) return TL_ERR_ARG; g_streamq_x3 = (int)value; return TL_OK; }
  if (!strcmp(key, "small_rows")) { g_small_rows = value; return TL_OK; }
  if (!strcmp(key, "small_mode")) { g_small_mode = (int)value; return TL_OK; }
  if (!strcmp(key, "wgrad_dense")) { g_wgrad_dense = (int)value; return TL_OK; }
  if (!strcmp(key, "wgrad_rows")) { g_wgrad_rows = (int)value; return TL_OK; }
  if (!strcmp(key, "wgrad_dma")) { g_wgrad_dma = (int)value; return TL_OK; }
  if (!strcmp(key, "wgrad_dense_min_rows")) { g_wgrad_dense_min_rows = value; return TL_OK; }
  return TL_ERR_ARG;
}

int tl_conv_fwd(const tl_conv_args* a, tl_stream_t stream) {
  if (!a || !a->in || !a->weight || !a->out || a->n_out <= 0 || a->K <= 0 || a->K > 27 || a->Cin <= 0 || a->Cout <= 0) return TL_ERR_ARG;
  const bool has_blk = a->blk_unit && a->blk_counter && a->blk_halo && a->blk_lrb && a->K == 27;
  const int bad = validate(a, has_blk);
  if (bad != TL_OK) return bad;
  Conv c;
  c.a = a; c.p = fill_convp(a, has_blk); c.al = conv_align(a); c.has_blk = has_blk; c.s = tl_s(stream);
  // float16: the same kernel sources compiled a second time with IEEE-half conversions (tl_half.h); inside those units -- and in the
  // rungs -- "TL_BF16" stands for "the 16-bit type"
  c.f16 = a->dtype == TL_F16;
  c.dt = c.f16 ? TL_BF16 : a->dtype;
  c.L = c.f16 ? &kTlConvF16 : &kTlConvBf16;
  c.train = a->epi_mode != TL_EPI_NONE;
  if (c.train && a->red_nparts) *a->red_nparts = 0;
  for (auto rung : kLadder) {
    const int rc = rung(c);
    if (rc != TL_NEXT) return rc;
  }
  return TL_ERR_UNSUPPORTED;                       // (not reached: the last rung always answers)
}

int tl_conv_route(const tl_conv_args* a, char* buf, int cap) {
  if (!buf || cap <= 0) return TL_ERR_ARG;
  TlRoute r;
  struct Armed {                                   // disarms on every return path
    explicit Armed(TlRoute* q) { tl_route_armed = q; }
    ~Armed() { tl_route_armed = nullptr; }
  } armed(&r);
  const int rc = tl_conv_fwd(a, nullptr);
  snprintf(buf, (size_t)cap, "%s", r.text);
  return (r.truncated || r.len >= cap) ? TL_ERR_ARG : rc;     // (a route that does not fit is cut, never reported as whole)
}

int64_t tl_conv_red_parts(int64_t n_out) {
  // the stream kernels write one row per 256 output rows, the persistent direct kernels at most 2048
  const int64_t a = tl_cdiv(n_out > 0 ? n_out : 1, 256);
  return a > 2048 ? a : 2048;
}

}  // extern "C"
