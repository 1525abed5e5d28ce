/* libgfv - C ABI of the MI355X-native (gfx950) Gen-FVGN hot path.
 *
 * Every entry point is `extern "C"`, takes plain device pointers + sizes + a hipStream_t (as void*), allocates
 * nothing, is asynchronous on the given stream and returns 0 (GFV_OK) or a negative error code.  State the library keeps:
 * the product form (a process-wide default, gfv_set_f16split, with an optional per-thread override,
 * gfv_set_f16split_thread) and the model's hidden size (thread-local, gfv_set_hidden_size - like the HIP runtime's current
 * device); a chain launch may carry its own of both in its argument struct,
 * the device status word (gfv_status_flags), the optional profiling records (gfv_profile_*) and the mesh plans a caller
 * creates and destroys (gfv_plan_create / gfv_plan_destroy).  All floating point data is fp32, all index data int32 (plans are narrowed from the reference's
 * int64 once per mesh batch).
 *
 * What each entry replaces in the reference (paths relative to /root/reference/src) is cited per function; the
 * reference has no native code of its own: these replace the third-party CUDA kernels it reaches through
 * torch_scatter / ATen / cuBLAS / Inductor.
 */
#ifndef GFV_H_
#define GFV_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): gfv_rowtile_args_t grew (rc_Wh, rc_bias; round 3 had already turned its former pad fields hidden / flags /
 * product_form into live inputs and appended fin_stats .. dw_in_ld without a bump), gfv_set_f16split became a process-wide
 * default with gfv_set_f16split_thread beside it.  A binding checks gfv_abi_version() AND gfv_struct_size() at load. */
/* 3 (round 6): buffer-size contracts that moved in round 5 without a bump are now part of the version - (1) ln_partial of a
 * GFV_IN_LNBWD / GFV_FIN_LNBWD launch and of gfv_trans_mlp_bwd must hold gfv_rowtile_ln_rows(M) = ceil(M / 32) rows (ABI 2 said
 * gfv_rowtile_tiles(M) = ceil(M / 64): the small-tile backward families fill one row per 32 rows); (2) a fused dw_partial launch
 * writes blocks 0 .. gfv_rowtile_dw_partials_m(M) - 1 ONLY (ABI 2 callers reduced gfv_rowtile_dw_partials() blocks: the blocks
 * beyond that count are NOT written and hold whatever the buffer held); (3) the status word has an asynchronous mirror
 * (gfv_status_mirror / gfv_status_publish) and gfv_adam_step_dev publishes it; Adam is one launch (state[16], gfv_adam_state_init;
 * gfv_adam_tick_dev / gfv_adam_update_dev removed); (4) new entry points
 * gfv_prep_stats / gfv_prep_apply, gfv_fvm_fwd_fused / gfv_fvm_bwd_fused, gfv_slice_token_attention_fwd / _bwd. */
#define GFV_ABI_VERSION 3
int gfv_abi_version(void);
/* sizeof of the argument structs as the library was compiled (which: 0 gfv_seg_t, 1 gfv_layer_t, 2 gfv_rowtile_args_t,
 * 3 gfv_wimg_desc_t, 4 gfv_dw_tile_t, 5 gfv_reduce_piece_t, 6 gfv_plan_desc_t, 7 gfv_trans_mlp_t, 8 gfv_trans_mlp_bwd_t,
 * 9 gfv_fvm_mesh_t, 10 gfv_renew_rec_t): lets a
 * binding check its own layout */
int gfv_struct_size(int32_t which);

/* ------------------------------------------------------------------------------------------------------------
 * Segmented (CSR) gather-reduce:  out[r,:] = scale[r] * sum_{k in [rowptr[r],rowptr[r+1])} src[col[k],:]
 * Atomics-free wavefront segmented reduce.  Replaces torch_scatter.scatter_add / scatter_mean and the fused
 * "gather then scatter" pairs at FVMmodel/Models/FVGN/blocks.py:35-51,92-99 and the index_put_ backward of
 * the gathers at blocks.py:101-102.  src is [n_src, F] row-major (ld = F), F in {4,8,...,256} multiple of 4,
 * or any F through the scalar path.  scale (per destination row) and src_scale (per source row, applied to
 * each gathered row) may be NULL.  `accumulate` != 0 adds into out.
 * ---------------------------------------------------------------------------------------------------------- */
int gfv_seg_gather_sum(const float* src, const int32_t* rowptr, const int32_t* col, const float* scale,
                       const float* src_scale, float* out, int32_t n_rows, int32_t F, int32_t accumulate, void* stream);

/* same; nnz_hint = rowptr[n_rows] if the caller knows it (only used for the profiler's algorithmic-byte count) */
int gfv_seg_gather_sum_nnz(const float* src, const int32_t* rowptr, const int32_t* col, const float* scale,
                           const float* src_scale, float* out, int32_t n_rows, int32_t F, int32_t accumulate,
                           int64_t nnz_hint, void* stream);

/* same; n_src_hint = rows of src (the distinct source rows: what SURVEY.md 8(d) prices a gather by); profiler only */
int gfv_seg_gather_sum_ex(const float* src, const int32_t* rowptr, const int32_t* col, const float* scale,
                          const float* src_scale, float* out, int32_t n_rows, int32_t F, int32_t accumulate,
                          int64_t nnz_hint, int64_t n_src_hint, void* stream);

/* Round 6.  The same reduce over the 64-column HALVES of 128-wide rows (half-row c = row c >> 1, columns 64 (c & 1) ...: the view
 * blocks.py:35-42 scatters to the two end nodes of an edge), with LayerNorm applied on the way in:
 *   out[r, :] = sum_k LN(y)[half-row col[k]],   LN(y)[e, c] = (y[e, c] - mean_e) * rstd_e * gamma[c] + beta[c],
 * y [*,128] = the pre-LayerNorm rows a chain launch saved (gfv_rowtile_args_t.fin_presave), stats [*,2] = its (mean, 1 / std)
 * (fin_stats).  The expression is the chain launch's own, so the sums equal - bit for bit - those over its LayerNorm output,
 * which the EdgeBlock forward then need not write a second time without the residual (512 B per edge row).  out [n_rows, 64];
 * y, gamma, beta, out 16-byte aligned.  The two hints: as gfv_seg_gather_sum_ex (profiler only). */
int gfv_seg_gather_sum_ln(const float* y, const float* stats, const float* gamma, const float* beta, const int32_t* rowptr,
                          const int32_t* col, float* out, int32_t n_rows, int64_t nnz_hint, int64_t n_src_hint, void* stream);

/* out[e, 0:F] = a[s[e], :], out[e, F:2F] = a[r[e], :]  (+ base[e,:] if base != NULL).  Adjoint of the
 * chunked edge->node scatter at blocks.py:34-42. */
int gfv_gather_pair(const float* a, const int32_t* s, const int32_t* r, const float* base, float* out,
                    int32_t n_edges, int32_t F, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused GEMM chain: up to three Linear layers applied to a tile of rows, with gather / concat / segmented-sum / LayerNorm
 * prologues and bias / GELU / LayerNorm / residual epilogues; forward and the dX chain of the backward are the same entry
 * with different element ops.  One entry point, several kernel families behind it (gfv_rowtile_last_path tells which):
 * the register-resident row-owner chain (a wave owns 16 rows; split-fp16 products from per-step weight images, or fp32
 * MFMA), the column-owner persistent backward with fused weight gradients (dw_partial) and the lean kernel for single-layer
 * launches.  ACCEPTED SHAPES (anything else returns GFV_ERR_ARG and launches nothing - the generic LDS kernel that used to take
 * the rest was retired with ABI 2; tests/test_kernels_gpu.py holds the negative test):
 *   plain:   every segment width a multiple of 32 and every row stride (seg ld, out_ld, res_ld) a multiple of 4; K and ldw of
 *            every layer multiples of 4; inner layers 128 wide, the last layer a multiple of 64 (exactly 128 with a LayerNorm
 *            epilogue).  Only this class takes LayerNorm backward (GFV_IN_LNBWD / GFV_FIN_LNBWD), segmented-sum segments
 *            (csr_rowptr) and per-segment saves.
 *   ragged:  any segment width / row stride, any first-layer K, a last layer of any width <= 128 (or a multiple of 64 above);
 *            inner layers 128 wide with K = 128; NO LayerNorm backward; a last layer that is not a multiple of 16 wide takes
 *            neither GFV_OP_MUL_DGELU nor a LayerNorm epilogue nor out_nores; GFV_IN_LN and gadd need a 128-wide seg[0] with a
 *            row stride that is a multiple of 4.
 * Replaces nn.Linear/GELU/LayerNorm inside build_mlp (FVMmodel/Models/FVGN/EPD.py:10-63), the concat + MLP of
 * EdgeBlock/NodeBlock (blocks.py:54,101-111) and the Linear layers of the Transolver block
 * (FVMmodel/Models/GraphTransolver/GraphTransolver.py:54-59,95,98-128,163-169).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
  const float* ptr;   /* [rows, ld] */
  const int32_t* idx; /* optional row gather index [M]; NULL = identity */
  int32_t width;      /* valid columns (<= 128); zero padded to a multiple of 16 inside the kernel */
  int32_t ld;         /* row stride in floats */
  /* optional segmented-sum segment (register-resident chain, no LayerNorm backward, widths multiples of 32):
   *   row m = csr_scale[m] * sum_{k in [csr_rowptr[m], csr_rowptr[m+1])} ptr[idx[k] * ld + 0:width]
   * (idx is then the CSR column list [nnz]; csr_scale may be NULL) - the GnBlock's neighbour aggregation
   * (blocks.py:25-51,84-99: scatter_add / scatter_mean over the two-way edge list) and the per-side scatter of the factored
   * EdgeBlock's adjoint as the prologue of the launch that consumes them, entries added in CSR order. */
  const int32_t* csr_rowptr;
  const float* csr_scale;
  float* save;        /* optional [M, 128]: the assembled rows of this segment (columns >= width are written as zeros) */
} gfv_seg_t;

enum {                /* per-layer element op applied to the accumulator */
  GFV_OP_NONE = 0,      /* v = acc + bias                                   */
  GFV_OP_BIAS_GELU = 1, /* v = acc + bias; save v; next input = gelu(v)     */
  GFV_OP_MUL_DGELU = 2  /* v = acc * gelu'(aux); save v; next input = v     */
};
enum { GFV_IN_NONE = 0, GFV_IN_GELU = 1, GFV_IN_LN = 2, GFV_IN_LNBWD = 3 };
/* gfv_rowtile_args_t.flags: the split-fp16 form has two kernel families - the row-owner chain (a wave owns 16 rows, weights
 * stream through LDS) and the column-owner persistent chain (a wave owns 16 columns, weights stay in registers for the whole
 * launch; 3-layer MLP launches).  By default big launches of a covered shape take the second. */
enum { GFV_CHAIN_ROW_OWNER = 1,     /* never the column-owner family */
       GFV_CHAIN_COLUMN_OWNER = 2   /* the column-owner family whatever the row count (if the shape is covered) */ };
enum { GFV_FIN_PLAIN = 0, GFV_FIN_LN = 1, GFV_FIN_LNBWD = 2 };

typedef struct {
  const float* W;     /* [N, K] row-major: nn.Linear weight (forward) or its transpose (dX chain); NULL only with Wh: a
                       * virtual layer whose 128-row passes come from different weight blocks, image = their images back to back */
  const float* bias;  /* [N] or NULL */
  int32_t K, N;       /* K = input width, N = output width (128 for inner layers; last layer: <= 384) */
  int32_t op;
  int32_t ldw;        /* row stride of W in floats; 0 = K (a column block of a wider weight: W1[:, 256:384]) */
  float* save;        /* optional [M, N] */
  const float* aux;   /* [M, N] for GFV_OP_MUL_DGELU */
  const void* Wh;     /* optional: split-fp16 image of W (gfv_weight_images); when every layer of a launch has one
                       * (and args.wmax is set) the products run on the f16 MFMA pipe, see below */
  const float* bias2; /* optional: bias of output columns >= 128 (a last layer whose two 128-row passes come from
                       * different Linear layers); NULL = bias[128..] */
} gfv_layer_t;

typedef struct {
  int32_t M;
  int32_t nseg;
  gfv_seg_t seg[3];       /* input row m = concat_i seg[i][idx_i[m], 0:width_i] */
  const float* in_add;    /* optional: seg[0] row += in_add row (same idx / ld as seg[0]) */
  int32_t in_op;
  int32_t nlayers;
  const float* in_gamma;  /* GFV_IN_LN / GFV_IN_LNBWD */
  const float* in_beta;
  const float* in_aux;    /* GFV_IN_LNBWD: the pre-LayerNorm values y [M,128] */
  const float* gadd;      /* optional [*,64]: input row m += [gadd[gadd_s[m]] | gadd[gadd_r[m]]] (before in_op) */
  const int32_t* gadd_s;
  const int32_t* gadd_r;
  float* in_save;         /* optional [M,128]: result of the prologue */
  float* ln_partial;      /* GFV_IN_LNBWD / GFV_FIN_LNBWD: [n_tiles, 2, 128] per-tile (dgamma, dbeta) partial sums; provide
                           * gfv_rowtile_ln_rows(M) rows, sum the first gfv_rowtile_last_ln_rows() of them (below) */
  gfv_layer_t layer[3];
  int32_t fin_op;
  int32_t hidden;         /* hidden_size of the model this launch belongs to (LayerNorm width; gfv_set_hidden_size); 0 = the calling
                           * thread's setting.  (Inside the library the launcher always fills it in for the kernel.) */
  const float* fin_gamma;
  const float* fin_beta;
  const float* fin_aux;   /* GFV_FIN_LNBWD: the LayerNorm input rows [M,128] */
  float* fin_presave;     /* GFV_FIN_LN: pre-LayerNorm values [M,128] */
  const float* res[3];    /* optional addend per 128-wide output chunk */
  int32_t res_ld[3];
  int32_t out_ld[3];
  float* out[3];          /* output pointer per 128-wide chunk of the last layer */
  float* out_nores;       /* optional [M,128]: chunk 0 result BEFORE the residual addend (EdgeBlock output e') */
  /* optional gathered addend to the FIRST layer's pre-activation (needs nlayers >= 2):
   *   z1[m, c] += padd[padd_s[m], c] + padd[padd_r[m], 128 + c],  c < 128,  padd = [*, padd_ld >= 256].
   * EdgeBlock first layer factored through the nodes: W1 [x_s | x_r | e] = (W1a x)[s] + (W1b x)[r] + W1c e
   * (blocks.py:54 concat + EPD.py:21 Linear), the two node-level products are computed once per node. */
  const float* padd;
  const int32_t* padd_s;
  const int32_t* padd_r;
  int32_t padd_ld;
  int32_t flags;          /* GFV_CHAIN_*: which kernel family may take the launch (0: the library decides by shape and size) */
  const float* wmax;      /* device scalar max|W| the layers' Wh images were built with (gfv_weight_images) */
  /* optional, written by the split-fp16 form only (gfv_rowtile_last_path() >= 5): per group of 16 consecutive rows the
   * exact power of two s with s * max|v| in [2^13, 2^14) of the gradient rows this launch leaves for the weight-gradient
   * kernel - slot 0: the prologue result (in_save), slot l + 1: layer l's saved GFV_OP_MUL_DGELU product, slot nlayers
   * (nlayers <= 2): output chunk 0.  Layout gscale[slot * gscale_ld + row / 16], gscale_ld >= ceil(M / 16).
   * gfv_dw_tile_t.gscale takes a slot: the slab scale of the gradient rows then needs no extra pass over them. */
  float* gscale;
  int32_t gscale_ld;
  int32_t product_form;   /* 0 = gfv_f16split_enabled() of the calling thread; 1 fp32 MFMA, 2 split-fp16, 3 / 4 reduced precision (fp16 / bf16) */
  /* LayerNorm statistics of the rows, [M, 2] = (mean, 1 / sqrt(var + eps)): written by a GFV_FIN_LN launch when fin_stats is
   * given, read by a GFV_IN_LNBWD launch when in_stats is given (the column-owner backward needs them: its LayerNorm backward
   * is spread over eight waves and takes the row statistics as they were in the forward instead of recomputing them) */
  float* fin_stats;
  const float* in_stats;
  /* Weight gradients fused into a dX chain (column-owner family only; gfv_rowtile_fuses_dw() tells whether a launch takes
   * it).  A backward chain [W3^T (x gelu'(z2)), W2^T (x gelu'(z1)), W1^T] holds, tile by tile, exactly the operands of the
   * weight gradients of the forward's third and second Linear:  dW3 = g3^T gelu(z2),  dW2 = gz2^T gelu(z1)  (g3 = the
   * prologue result, gz2 = layer 0's product, z2 / z1 = layer[0].aux / layer[1].aux), their bias gradients (column sums of
   * g3 / gz2) and the LayerNorm's (dgamma, dbeta).  With dw_partial set the launch accumulates them per workgroup - no float
   * atomics - and leaves  dw_partial[wg * dw_partial_stride + ...] = [dW3 (128 x 128, row n, column k) | db3 (128) | dW2 |
   * db2 | dgamma | dbeta]  (GFV_DW_FUSED_FLOATS floats) for wg < gfv_rowtile_dw_partials_m(M); sum them with gfv_reduce_multi.
   * BLOCKS AT OR BEYOND gfv_rowtile_dw_partials_m(M) ARE NOT WRITTEN (ABI 3; until round 5 a launch zero-filled all
   * gfv_rowtile_dw_partials() blocks): reduce exactly gfv_rowtile_dw_partials_m(M) of them.
   * layer[0].save / in_save / ln_partial may then be NULL (nothing else reads g3 / gz2). */
  float* dw_partial;
  int64_t dw_partial_stride;
  /* RESERVED (ABI 3): rounds 3 - 5 took the input rows of the forward's first Linear here and fused that weight gradient as well
   * (GFV_DW_FUSED_FLOATS_IN floats per block) - time-neutral at its best (profiles/r05_ab_dw1_trailing.txt), removed with its
   * kernel instantiations.  Must be NULL / 0: a launch with dw_in set does not run fused (gfv_rowtile_fuses_dw says 0). */
  const float* dw_in;
  int32_t dw_in_ld;
  int32_t reserved2_;
  /* optional with dw_partial (ABI 2): RECOMPUTE instead of re-read.  rc_Wh[0] / rc_Wh[1] = split-fp16 images (built with the
   * same wmax) of the FORWARD's second and third Linear ([128, 128] each, un-transposed), rc_bias[0] / rc_bias[1] their biases
   * (or NULL).  The launch then rebuilds z2 = W2 gelu(z1) + b2 and the LayerNorm input y = W3 gelu(z2) + b3 tile by tile from
   * z1 (layer[1].aux) on the matrix cores; layer[0].aux (z2) and in_aux (y) are NOT read and may be NULL - the forward launch
   * need not save them (gfv_layer_t.save of its second layer, fin_presave).  in_stats is still read (the rows' forward
   * statistics). */
  const void* rc_Wh[2];
  const float* rc_bias[2];
} gfv_rowtile_args_t;
enum { GFV_DW_FUSED_FLOATS = 2 * 128 * 128 + 4 * 128 };
int gfv_rowtile_dw_partials(void);                              /* the most workgroups (= partial blocks) a fused launch runs */
int gfv_rowtile_dw_partials_m(int32_t M);                       /* ... a fused launch over M rows runs: blocks 0 .. this - 1 are written */
int gfv_rowtile_fuses_dw(const gfv_rowtile_args_t* args);       /* 1: gfv_rowtile_chain would run this launch with fused weight gradients */

int gfv_rowtile_tiles(int32_t M); /* number of 64-row tiles = rows of ln_partial every family but the small-tile backward fills */
/* rows of ln_partial to PROVIDE for a launch over M rows (one per 32 rows), and how many of them the calling thread's last
 * gfv_rowtile_chain launch filled: ceil(M / 32) when the column-owner small-tile backward took it (csrc/cbwd.hip; last_path & 128),
 * gfv_rowtile_tiles(M) otherwise.  The rows beyond that count are not written. */
int gfv_rowtile_ln_rows(int32_t M);
int gfv_rowtile_last_ln_rows(void);
/* Dispatch limits (round 6): which kernel family takes a launch of M rows is decided by ONE table (csrc/gfv_limits.h lists the
 * entries: GFV_CBWD_MAX_M, GFV_CFWD_TG2_MAX_M, GFV_CFWDP_MIN_M ...).  A limit takes the value of the environment variable of its
 * name ONCE, at first use (or its built-in default); gfv_set_limit moves it afterwards (value < 0: back to environment / default) -
 * process-wide, for tests and A/B tools.  gfv_limit_name(which) = the variable's name, NULL past the last entry. */
int gfv_get_limit(int32_t which);
int gfv_set_limit(int32_t which, int32_t value);
const char* gfv_limit_name(int32_t which);
int gfv_rowtile_chain(const gfv_rowtile_args_t* args, void* stream);
/* which kernel the calling thread's last gfv_rowtile_chain launch took: 1 register-resident chain, 2 its ragged-shape
 * instantiation (0 was the generic LDS row-tile kernel, retired with ABI 2); + 4 when the products ran as split-fp16; + 8 when the column-owner persistent
 * family took the launch, + 16 when it ran with fused weight gradients, + 32 when a single-layer launch ran on the lean
 * one-Linear kernel (csrc/lin1.hip: the layer's image staged in LDS once per 128-row workgroup; same products, same
 * results to rounding), + 64 when a short 3-layer LayerNorm forward ran on the column-owner small-tile kernel (csrc/cfwd.hip:
 * a wave owns 32 output columns of a 32- / 64-row tile; hidden activations split behind a fixed scale as in the column-owner
 * backward), + 128 when a short dX chain behind a LayerNorm backward (in_stats given, no fused weight gradients) ran on the
 * column-owner small-tile backward (csrc/cbwd.hip: 32- / 64-row tiles on 8 waves, the scales of the persistent backward)
 * (tests assert the path they mean) */
int gfv_rowtile_last_path(void);

/* fp32 products on the f16 MFMA pipe (v_mfma_f32_16x16x32_f16, 16x the f32 MFMA rate): every fp32 operand is split
 * into two fp16 parts, x = hi + lo (22 mantissa bits after an exact power-of-two scaling: per input row for the
 * activations, one global scale 2^s from max|W| for the weights), and hi*hi + hi*lo + lo*hi is accumulated in fp32 -
 * 3 MFMAs instead of 8, error <= that of the f32 MFMA (products are exact, the dropped lo*lo term is 2^-22 relative).
 * The weights are split once per step into an image in MFMA-fragment order:
 *   image[pass = n/128][T = k/32][nt = (n%128)/16][part][lane = 16 g + i][e]  (fp16),
 *   element = part(2^s W[128 pass + 16 nt + i][32 T + 16 (e>>2) + 4 g + (e&3)]),  zero outside [N, K]
 * (16 KB per (pass, T): exactly the LDS slice the chain kernel streams).  The activations are split in registers. */
typedef struct {
  const float* W; /* [N, K], row stride ldw */
  void* img;      /* gfv_weight_image_bytes(N, K) bytes */
  int32_t ldw, N, K, reserved;
} gfv_wimg_desc_t;
size_t gfv_weight_image_bytes(int32_t N, int32_t K);
/* wmax[0] = max |W| over all described blocks (device scalar, overwritten) */
/* the product form of the launches that do not name their own: a PROCESS-WIDE default (initial value: environment
 * GFV_F16SPLIT, default 1; gfv_set_f16split) - it must reach launches issued from other threads than the one that chose it:
 * PyTorch runs the backward of an autograd node on its device worker thread - and an optional override of the CALLING THREAD
 * (gfv_set_f16split_thread(0 / 1 / 2 / 3); -1 removes it) for hosts that drive two models in different forms from two threads.
 * gfv_set_f16split also removes the calling thread's override.  gfv_f16split_enabled() = what a launch from this thread gets.
 * 0 = fp32 MFMA everywhere (chain launches ignore their images, weight gradients take the fp32 kernel);
 * 1 = split-fp16 products (fp32 accuracy);
 * 2 = reduced precision: one fp16 x fp16 product per term with fp32 accumulation - the high parts of the same operands
 *     (11 significand bits: results agree with the fp32 forms to ~1e-3; the counterpart of the reference's autocast runs,
 *     BASELINE configs 3 / 5 - never the form the parity claims or bench.py's `value` are made on);
 * 3 = the same single product with bf16 operands (v_mfma_f32_16x16x32_bf16, fp32 accumulation; 8 significand bits: ~1e-2 of
 *     the fp32 forms) - BASELINE config 3's "bf16 MLP GEMMs on MFMA" to the letter.  Same fragment layouts and scales; the
 *     weight images hold bf16 high parts and no low parts, so they must be BUILT in this form: gfv_weight_images reads the
 *     calling thread's form, and images built in forms 0 - 2 are not valid for form 3 (nor the other way round). */
int gfv_f16split_enabled(void);
int gfv_set_f16split(int32_t on);
int gfv_set_f16split_thread(int32_t on);
/* hidden_size of the model the following launches belong to (the reference's --hidden_size, utils/get_param.py:69; default
 * 128; multiples of 16 in [16, 128]).  Every kernel works on 128-column latent rows; a narrower model runs zero-padded to
 * 128 columns (the host side pads its parameters: FVMmodel/padding.py) and differs in two places only - LayerNorm takes its
 * statistics over the h real columns, and the slice attention scales by (h / 8) ** -0.5.  Thread-local host state read by
 * the launchers: set it before the launches of a model (gfv.engine.Engine does, on every forward and backward); a chain
 * launch may name its own (gfv_rowtile_args_t.hidden).
 * PRECONDITION at h < 128: the padded columns of every LayerNorm input are EXACTLY zero (zero-padded weights, biases, gamma and
 * beta keep them so).  No launch is told where the h real columns sit (node latents 0 .. h - 1, the halves of an edge latent
 * at 0 and 64): the statistics are mean = sum_128 / h and sum_sq = sum over the NON-ZERO entries of (x - mean)^2 + (number of
 * zero entries - (128 - h)) mean^2 - a zero beyond the 128 - h padded ones is a real column that deviates by -mean.  A non-zero
 * value in a padded column is counted as a real one.  h = 128 runs kernels of its own, which hold the plain sum only. */
int gfv_hidden_size(void);
int gfv_set_hidden_size(int32_t h);
int gfv_weight_absmax(const gfv_wimg_desc_t* descs_dev, int32_t n_desc, float* wmax, void* stream);
/* build every image; max_frags = max over descs of gfv_weight_image_bytes / 32 */
int gfv_weight_images(const gfv_wimg_desc_t* descs_dev, int32_t n_desc, int64_t max_frags, const float* wmax,
                      void* stream);
/* The form tag of a set of images: -1 = `wmax` is not the scale of images this library built, 0 = fp16 (hi, lo) parts (built in
 * forms 0 / 1 / 2), 1 = bf16 high parts (built in form 3).  Kept per `wmax` address (host state, set by gfv_weight_images);
 * gfv_rowtile_chain and gfv_trans_mlp_fwd / _bwd return GFV_ERR_ARG for a launch whose product form is of the other class than
 * the images it names through args.wmax - images carry nothing in their bytes that would tell. */
int gfv_weight_images_form(const float* wmax);

/* Weight gradient of a Linear layer: dW[n,k] = sum_m G[m,n] * A[m,k], db[n] = sum_m G[m,n] (two-stage,
 * deterministic).  A is assembled like the forward input (segments, gather, optional GELU of a saved
 * pre-activation).  partial: workspace [gfv_dw_chunks(M), N(=128), Kpad] (+ N floats per chunk for db).
 * M = 0 (no rows) is legal: accumulate = 0 writes zeros to dW and db, accumulate = 1 leaves them unchanged; nothing else is
 * launched and the workspace is neither read nor written.
 * Replaces the autograd mm/addmm wgrad of nn.Linear (pre_train_Adam.py:188). */
int gfv_dw_chunks(int32_t M);
int gfv_linear_dw(const float* G, int32_t ldg, int32_t n_out, const gfv_seg_t* segs, int32_t nseg,
                  const float* in_add, int32_t a_gelu, int32_t M, float* dW, float* db, float* workspace,
                  int32_t accumulate, void* stream);
/* same as _ex, with the per-16-row scales of the G rows handed over (gfv_dw_tile_t.gscale; NULL = none) */
int gfv_linear_dw_gs(const float* G, int32_t ldg, int32_t n_out, const gfv_seg_t* segs, int32_t nseg,
                     const float* in_add, int32_t a_op, const float* a_gamma, const float* a_beta, int32_t M,
                     float* dW, const float* gscale, float* db, float* workspace, int32_t accumulate, void* stream);
size_t gfv_linear_dw_workspace_floats(int32_t M, int32_t n_out, int32_t K);
/* same, with the input-row op spelled out: a_op 0 none, 1 GELU, 2 LayerNorm(a_gamma, a_beta) (single 128-wide segment) */
int gfv_linear_dw_ex(const float* G, int32_t ldg, int32_t n_out, const gfv_seg_t* segs, int32_t nseg,
                     const float* in_add, int32_t a_op, const float* a_gamma, const float* a_beta, int32_t M,
                     float* dW, int32_t reserved, float* db, float* workspace, int32_t accumulate, void* stream);

/* All weight gradients of one fused MLP (or any set of <= 6 output tiles) in ONE launch + ONE reduction.
 * Tile t: dW_t[n,k] = sum_m G_t[m,n] * op(A_t[idx_t[m], k]) for n < n_out, k < width, written at
 * block[out_off + n*ld_out + k]; if db_off >= 0 also block[db_off + n] = sum_m G_t[m,n].  `grad_block` is the
 * contiguous gradient storage of the parameter block ([W1|b1|W2|b2|W3|b3] in state_dict order, each tensor padded
 * to a multiple of 4 floats), block_floats its length.  workspace: gfv_dw_multi_workspace_floats(...) floats,
 * zero-initialised once by the caller (padding slots are never written).
 * M = 0: the workspace is not touched; a grad_block is zeroed (all block_floats of it) with accumulate = 0 and left unchanged with
 * accumulate = 1; with grad_block == NULL there are no slabs (gfv_dw_slabs returns 0) and nothing for the caller to reduce. */
typedef struct {
  const float* G;       /* [M, ldg] upstream gradient rows */
  const float* A;       /* input rows [*, ld] */
  const int32_t* idx;   /* optional gather index for A rows */
  const float* in_add;  /* optional second addend for A (same idx / ld) */
  const float* a_gamma; /* a_op == 2 */
  const float* a_beta;
  int32_t ldg, n_out, width, ld;
  int32_t a_op;         /* 0 none, 1 GELU, 2 LayerNorm(a_gamma, a_beta) (width 128); | GFV_DW_COLSCALE (with 0 only) */
  int32_t ld_out;       /* row stride (K of the weight) inside the block */
  int64_t out_off;      /* float offset of dW_t[0, 0] inside the block */
  int64_t db_off;       /* float offset of the bias gradient, or -1 */
  const float* gscale;  /* optional (split-fp16 form): per-16-row power-of-two scales of the G rows as the chain launch
                         * that produced them wrote them (gfv_rowtile_args_t.gscale); NULL: one pass over G finds the maximum */
} gfv_dw_tile_t;
/* Range of the split-fp16 weight-gradient form.  The gradient rows G carry ONE power of two per slab of rows.  The
 * activations A carry one power of two per COLUMN and slab when the tile asks for it (a_op = 0 | GFV_DW_COLSCALE: a pass
 * over the slab's A rows finds the column maxima - encoder inputs hold geometric columns at mesh-spacing scale next to O(1)
 * features); otherwise they are split unscaled (latent rows, GELU / LayerNorm outputs: O(1)), and a value beyond the fp16
 * range raises GFV_FLAG_DW_RANGE in the device status word instead of being clamped. */
enum { GFV_DW_COLSCALE = 8 };
enum { GFV_FLAG_DW_RANGE = 1,
       /* column-owner chain family: a hidden activation beyond 2^11 (they are split after a fixed scale, see
        * csrc/colchain_kernel.h; GFV_COLCHAIN=0 keeps every launch on the row-scaled family) */
       GFV_FLAG_CHAIN_RANGE = 2 };
/* device status word: OR of GFV_FLAG_* raised by kernels since the last call; reads (synchronising) and clears it */
int gfv_status_flags(int32_t* flags_out);
/* The same word WITHOUT a synchronisation (round 6): *host_word = a pinned, device-mapped int32 the library owns (allocated at the
 * first call, one per process).  gfv_status_publish enqueues a one-thread kernel on `stream` that copies a non-zero status word
 * into it (the device word stays raised until gfv_status_flags clears it); gfv_adam_step_dev does the same from inside the Adam
 * launch once the mirror exists.  A host loop reads *host_word after the NEXT step was issued (the previous step's
 * kernels have long finished: no wait), and on a non-zero value calls gfv_status_flags (clears the device word), zeroes
 * *host_word and raises.  gfv.trainer.TrainStep.step and FVMmodel.importer.NNmodel.forward do exactly that (FloatingPointError). */
int gfv_status_mirror(int32_t** host_word);
int gfv_status_publish(void* stream);
int gfv_dw_slabs(int32_t M, int32_t ntiles, int32_t* rows_per_slab);
size_t gfv_dw_multi_workspace_floats(int32_t M, int32_t ntiles, int64_t block_floats);
int gfv_dw_multi(const gfv_dw_tile_t* tiles, int32_t ntiles, int32_t M, int64_t block_floats, float* workspace,
                 float* grad_block, int32_t accumulate, void* stream);

/* out[j] (+)= sum_c partial[c, j]  (c < n_chunks, j < n) */
int gfv_reduce_partials(const float* partial, int32_t n_chunks, int32_t n, float* out, int32_t accumulate,
                        void* stream);

/* 2-D form: out[r * ld_out + c] = sum_chunk partial[chunk * chunk_stride + r * cols + c] (r < rows, c < cols; cols, ld_out,
 * chunk_stride multiples of 4, 16-byte aligned): a [rows, cols] piece of the slab workspace of gfv_dw_multi reduced straight
 * into a column block of a wider gradient matrix.  gfv_dw_multi with grad_block == NULL leaves the reduction to the caller. */
int gfv_reduce_partials_2d(const float* partial, int32_t n_chunks, int64_t chunk_stride, int32_t rows, int32_t cols,
                           int32_t ld_out, float* out, void* stream);

/* Several such reductions in ONE launch (the parameter gradients of one MLP: slab partials of gfv_dw_multi with
 * grad_block == NULL, per-tile LayerNorm partials, small per-block partials), each straight into its place:
 *   out[r * ld_out + c] = sum_{chunk < n_chunks} partial[chunk * chunk_stride + r * ld_in + c]   (r < rows, c < cols)
 * cols, ld_in, ld_out, chunk_stride multiples of 4 floats, pointers 16-byte aligned; n_pieces <= 12.  Fixed summation
 * order (16 interleaved chunk lanes, then an ordered fold): deterministic, no atomics. */
typedef struct {
  const float* partial;
  float* out;
  int64_t chunk_stride; /* floats between consecutive chunks */
  int32_t n_chunks, rows, cols, ld_in, ld_out, reserved;
} gfv_reduce_piece_t;
int gfv_reduce_multi(const gfv_reduce_piece_t* pieces, int32_t n_pieces, void* stream);

/* Segmented form: out[b, 0:n] = sum of the chunk rows seg_ptr[b] .. seg_ptr[b+1]-1 of partial [n_chunks, n] (n % 4 == 0,
 * 16-byte aligned).  Pre-reduces the per-chunk slice tokens of each graph (GraphTransolver.py:64-73 global_add_pool). */
int gfv_reduce_partials_seg(const float* partial, const int32_t* seg_ptr, int32_t n_seg, int32_t n, float* out,
                            void* stream);

/* Batched form: one launch for all weight transposes of a step; `descs` [n] lives in DEVICE memory. */
typedef struct {
  const float* in; /* [rows, ld_in], columns [0, cols) are transposed */
  float* out;      /* [cols, ld_out] */
  int32_t rows, cols, ld_in, ld_out; /* ld_out: row stride of out, 0 = rows */
} gfv_transpose_desc_t;
int gfv_transpose_batch(const gfv_transpose_desc_t* descs, int32_t n, int32_t max_rows, int32_t max_cols, void* stream);

/* Batch assembly of the device-resident state pool (replaces the per-step host batching + H2D copy of
 * Load_mesh/Graph_loader.py:405-480,830-1006): descriptor i copies n_words 32-bit words src -> dst, kind 0 verbatim
 * (floats, ids), kind 1 adding `add` to every (int32) word (index offsets of the block-diagonal batch), kind 2 filling
 * `add` (graph id).  `descs` [n_desc] lives in DEVICE memory; one launch for the whole batch. */
typedef struct {
  const void* src;
  void* dst;
  int64_t n_words;
  int32_t kind;
  int32_t add;
} gfv_concat_desc_t;
int gfv_concat_offsets(const gfv_concat_desc_t* descs, int32_t n_desc, int32_t blocks_per_desc, void* stream);

/* out [cols, rows] = in^T for a [rows, cols] fp32 matrix with row stride ld_in (weights for the dX chain). */
int gfv_transpose(const float* in, int32_t ld_in, float* out, int32_t rows, int32_t cols, void* stream);


/* ------------------------------------------------------------------------------------------------------------
 * Transolver physics attention (H=8 heads, D=16, G=32 slices).  Replaces
 * FVMmodel/Models/GraphTransolver/GraphTransolver.py:61-95 (softmax slice weights, scatter_add slice tokens over
 * `batch`, 32x32 attention per (graph, head), de-slice) without materialising [N,8,32,16].
 * Layouts: xmid/fx/out_x [N,128] = [N,8,16]; w, gw [N,8,32]; tokens [B,8,32,16]; norm [B,8,32]; attn [B,8,32,32].
 * Node chunks: contiguous node ranges inside one graph (chunk_beg/chunk_end [n_chunks]; gchunk_ptr [B+1]).
 * ---------------------------------------------------------------------------------------------------------- */
int gfv_slice_softmax_fwd(const float* xmid, const float* Ws, const float* bs, const float* temp, float* w, int32_t N,
                          void* stream);
int gfv_slice_softmax_bwd_blocks(int32_t N); /* rows of `partial` ([blocks][552] = dWs 512 | dbs 32 | dT 8) */
int gfv_slice_softmax_bwd(const float* xmid, const float* Ws, const float* bs, const float* temp, const float* w,
                          const float* gw, float* gxmid, float* partial, int32_t N, void* stream);
/* partial[chunk][h*32+g][0:16] = sum_n w[n,h,g] a[n,h,:], [16] = sum_n w[n,h,g] */
int gfv_slice_token_partial(const float* w, const float* a, const int32_t* chunk_beg, const int32_t* chunk_end,
                            int32_t n_chunks, float* partial, void* stream);
/* (token, norm, attn: what the backward reads - each may be NULL in a forward-only step) */
int gfv_slice_attention_fwd(const float* partial, const int32_t* gchunk_ptr, int32_t B, const float* Wq, const float* Wk,
                            const float* Wv, float* token, float* norm, float* attn, float* out_token, void* stream);
/* dW_partial [B*8][3][16][16] (q,k,v), reduce with gfv_reduce_partials */
int gfv_slice_attention_bwd(const float* gpartial, const int32_t* gchunk_ptr, int32_t B, const float* Wq, const float* Wk,
                            const float* Wv, const float* token, const float* norm, const float* attn, float* g_raw,
                            float* g_norm, float* dW_partial, void* stream);
/* gfv_slice_softmax_fwd followed by gfv_slice_token_partial(w, a) in one pass (w is written out as well): the forward of
 * GraphTransolver.py:64-73 up to the per-chunk slice tokens, on the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32) */
int gfv_slice_softmax_token(const float* xmid, const float* Ws, const float* bs, const float* temp, const float* a,
                            const int32_t* chunk_beg, const int32_t* chunk_end, int32_t n_chunks, float* w, float* partial,
                            void* stream);
/* out[n,h,:] (+)= sum_g w[n,h,g] T[batch[n],h,g,:].  accumulate: bit 0 = add into out; bit 2 (value 4) = the batch is ONE
 * graph (spares the pass over workgroups that straddle two graphs) */
int gfv_deslice(const float* w, const float* T, const int32_t* batch, float* out, int32_t N, int32_t accumulate,
                void* stream);
/* gw[n,h,g] (+)= sum_c a[n,h,c] T[batch[n],h,g,c] + add[batch[n],h,g] */
int gfv_slice_gw(const float* a, const float* T, const float* add, const int32_t* batch, float* gw, int32_t N,
                 int32_t accumulate, void* stream);
/* Everything behind the attention adjoint of a Transolver block in one pass over the nodes (GraphTransolver.py:64-92,
 * backward): gw = gfv_slice_gw(g_out_x, out_token) + gfv_slice_gw(fx_mid, g_raw, g_norm) stays in registers, g_fx_mid =
 * gfv_deslice(w, g_raw), (g_x_mid, partial) = gfv_slice_softmax_bwd(.., gw) - the same terms in the same order as those
 * four launches (equal to rounding).  partial: gfv_slice_softmax_bwd_blocks(N) x 552 floats.  n_graphs: graphs in the batch
 * (1: every workgroup of 32 nodes lies in one graph and runs on the matrix cores, v_mfma_f32_16x16x4_f32 - exact fp32
 * products; otherwise the workgroups that straddle two graphs are taken by a second, scalar launch). */
int gfv_slice_post_bwd(const float* xmid, const float* Ws, const float* bs, const float* temp, const float* w,
                       const float* g_out_x, const float* out_token, const float* fx_mid, const float* g_raw,
                       const float* g_norm, const int32_t* batch, float* g_x_mid, float* g_fx_mid, float* partial,
                       int32_t N, int32_t n_graphs, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Finite-volume discretisation (conserved form).  Replaces FVMmodel/FVdiscretization/FVscheme.py:618-724,50-274,
 * FVgrad.py:235-367 (precomputed-moments branch), FVInterpolation.py:36-185,218-265 and the clamp / Dirichlet /
 * integrator mixing of FVMmodel/importer.py:187-201,223-231.  Padded layouts: phi [N,8] = (u,v,p,uh,vh,uo,vo,0),
 * grad [N,16] = d(phi_c)/d(x,y) at 2c+a, Ff [E,16] = (phi_f[0:5], grad_f[c][a] at 5+2c+a), cres [C,4] =
 * (div, Rx, Ry, sum |lp|^2), losses [B,4] = (cont, mom_x, mom_y, press).  mode: 0 explicit, 1 implicit, 2 imex.
 * ---------------------------------------------------------------------------------------------------------- */
int gfv_phi_fwd(const float* dec, const float* y, const int32_t* node_type, const float* uv_old, float* phi, int32_t N,
                int32_t mode, void* stream);
/* gfv_phi_fwd with a separate baseline of the time difference (gfv_time_scheme_update): uv_hat is still formed from uv_old (u_n,
 * what the input preparation wrote), channels 5 and 6 of phi carry uv_star.  gfv_phi_bwd is its adjoint too: the baseline carries
 * no gradient. */
int gfv_phi_fwd_ts(const float* dec, const float* y, const int32_t* node_type, const float* uv_old, const float* uv_star,
                   float* phi, int32_t N, int32_t mode, void* stream);
int gfv_phi_bwd(const float* gphi, const float* dec, const int32_t* node_type, float* gdec, int32_t N, int32_t mode,
                void* stream);
/* rowptr/outn/Bp: directed stencil in CSR order of the receiving node, Bp [S,5] permuted moment vectors;
 * An [N,25] the moment matrix A as the reference stores it (graph_node_x.A_node_to_node, fp32), rn [N,5] = its row norms
 * + 1e-8 (FVgrad.py:335).  The kernel forms A / rn, accumulates the right-hand side and runs the pivoted LU + solves in
 * DOUBLE: cond(A_n) reaches 4e5 on the reference's boundary-layer meshes, where an fp32 elimination (the reference's own
 * included) returns rounding noise of size cond * 2^-24; the exact solution of the fp32 data sits in the middle of it. */
int gfv_wlsq_fwd(const float* phi, const int32_t* rowptr, const int32_t* outn, const float* Bp, const float* An,
                 const float* rn, float* grad, int32_t N, void* stream);
/* adjoint; rowptr_o/inn/Bo: the same stencil in CSR order of the SENDING node, sumB [N,5]; grhs_ws [N,8,5];
 * adds into gphi */
int gfv_wlsq_bwd(const float* ggrad, const float* An, const float* rn, const int32_t* rowptr_o, const int32_t* inn,
                 const float* Bo, const float* sumB, float* grhs_ws, float* gphi, int32_t N, void* stream);
/* stand-alone node_based_WLSQ: all five 2nd-order derivative entries, full5 / g5 laid out [N,8,5]; 7 channels */
int gfv_wlsq_fwd_full(const float* phi, const int32_t* rowptr, const int32_t* outn, const float* Bp, const float* An,
                      const float* rn, float* grad, float* full5, int32_t N, void* stream);
int gfv_wlsq_bwd_full(const float* g5, const float* An, const float* rn, const int32_t* rowptr_o, const int32_t* inn,
                      const float* Bo, const float* sumB, float* grhs_ws, float* gphi, int32_t N, void* stream);
/* any reconstruction order (FVorder.py:23-72; row f4): terms = Taylor terms M = 2 (1st) / 5 (2nd) / 9 (3rd) / 14 (4th);
 * Bp / Bo [S,M], An [N,M*M], rn / sumB [N,M], grhs_ws [N,8,M].  full / gfull (optional) [N,8,M]: all M derivative entries
 * (7 channels) out of the forward / into the adjoint; the adjoint takes exactly one of ggrad [N,16] and gfull. */
int gfv_wlsq_fwd_ex(const float* phi, const int32_t* rowptr, const int32_t* outn, const float* Bp, const float* An,
                    const float* rn, float* grad, float* full, int32_t N, int32_t terms, void* stream);
int gfv_wlsq_bwd_ex(const float* ggrad, const float* gfull, const float* An, const float* rn, const int32_t* rowptr_o,
                    const int32_t* inn, const float* Bo, const float* sumB, float* grhs_ws, float* gphi, int32_t N,
                    int32_t terms, void* stream);
int gfv_face_fwd(const float* phi, const float* grad, const int32_t* es, const int32_t* er, const float* pos,
                 const float* fpos, const int32_t* ftype, const float* y, float* Ff, int32_t E, void* stream);
int gfv_cell_fwd(const float* phi, const float* grad, const float* Ff, const float* pos, const int32_t* crow,
                 const int32_t* kface, const int32_t* knode, const float* kS, const int32_t* ftype, const float* centroid,
                 const float* area, const int32_t* cbatch, const float* theta, const float* dt, const float* uvp_dim,
                 const float* sigma, float* phic, float* cres, float* uvp_cell, int32_t C, void* stream);
/* Same with the residuals of the NON-conserved form (FVscheme.py:276-511 as the reference calls it, hessian None):
 * continuity, convection and pressure terms from the cell means of the node gradients (saved to gradc [C,16]). */
int gfv_cell_fwd_ex(const float* phi, const float* grad, const float* Ff, const float* pos, const int32_t* crow,
                    const int32_t* kface, const int32_t* knode, const float* kS, const int32_t* ftype,
                    const float* centroid, const float* area, const int32_t* cbatch, const float* theta, const float* dt,
                    const float* uvp_dim, const float* sigma, float* phic, float* cres, float* uvp_cell, int32_t C,
                    int32_t non_conserved, float* gradc, void* stream);
int gfv_graph_loss(const float* cres, const int32_t* gcell_ptr, const float* theta, const float* sigma, float* sums,
                   float* losses, int32_t B, void* stream);
int gfv_cell_to_node(const float* phic, const int32_t* nrow, const int32_t* ncell, const float* pos, const float* centroid,
                     const int32_t* node_type, const float* y, const int32_t* nbatch, const float* uvp_dim,
                     const float* sigma, const float* phi, int32_t smooth, float* out, int32_t N, void* stream);
/* adjoint of face_fwd + cell_fwd + graph_loss: gloss [B,4] -> gphi [N,8], ggrad [N,16] (overwritten) */
int gfv_fvm_bwd(const float* cres, const float* sums, const float* gloss, const float* Ff, const int32_t* cbatch,
                const float* theta, const float* sigma, const float* dt, const int32_t* frow, const int32_t* fk,
                const int32_t* kcell, const float* kS, const int32_t* ftype, const int32_t* nfrow, const int32_t* nfcol2,
                const int32_t* nrow, const int32_t* ncell, const int32_t* crow, const float* pos, const float* fpos,
                const float* centroid, const float* area, float* gc_ws, float* gFf_ws, float* gphi, float* ggrad,
                int32_t N, int32_t E, int32_t C, void* stream);
int gfv_fvm_bwd_ex(const float* cres, const float* sums, const float* gloss, const float* Ff, const int32_t* cbatch,
                   const float* theta, const float* sigma, const float* dt, const int32_t* frow, const int32_t* fk,
                   const int32_t* kcell, const float* kS, const int32_t* ftype, const int32_t* nfrow, const int32_t* nfcol2,
                   const int32_t* nrow, const int32_t* ncell, const int32_t* crow, const float* pos, const float* fpos,
                   const float* centroid, const float* area, float* gc_ws, float* gFf_ws, float* gphi, float* ggrad,
                   int32_t N, int32_t E, int32_t C, int32_t non_conserved, const float* gradc, const float* phic,
                   void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Input normalisation / edge features / optimiser.  Replace FVMmodel/importer.py:54-93,114-130,166-178,
 * utils/normalization.py:32-85, torch.optim.Adam (pre_train_Adam.py:79,191) and the loss of
 * pre_train_Adam.py:177-184.
 * ---------------------------------------------------------------------------------------------------------- */
int gfv_graph_norm_stats(const float* x, int32_t ldx, const int32_t* gnode_ptr, int32_t B, float* stats, void* stream);
/* the same over 64 workgroups per graph (a single workgroup reads at the bandwidth of one CU): sums of x and x^2 in double per
 * workgroup, folded in a fixed order by a second small launch; workspace: gfv_graph_norm_workspace_bytes(B) bytes */
size_t gfv_graph_norm_workspace_bytes(int32_t B);
int gfv_graph_norm_stats_ws(const float* x, int32_t ldx, const int32_t* gnode_ptr, int32_t B, float* stats, void* workspace,
                            void* stream);
int gfv_normalizer_blocks(int32_t N);
int gfv_normalizer_update(const float* x, int32_t ldx, int32_t N, int32_t accumulate, float* acc_count, float* num_acc,
                          float* acc_sum, float* acc_sq, float* partial_ws, float* mean_std, void* stream);
int gfv_node_prep(float* x, int32_t ldx, const int32_t* batch, const float* stats, const float* uvp_dim,
                  const float* mean_std, int32_t norm_global, float* uv_old, int32_t N, void* stream);
int gfv_edge_attr(const float* x, int32_t ldx, const float* pos, const int32_t* es, const int32_t* er, float* out16,
                  float* out15, int32_t E, void* stream);
/* Round 6 - the input preparation as TWO launches (importer.py:114-130,166-178: was graph_norm_stats_ws + normalizer_update +
 * node_prep + edge_attr, and a state-restore copy in front of them in the solve loop, solve_with_grad_GPU.py:143).
 * gfv_prep_stats: stats[B,6] as gfv_graph_norm_stats_ws forms them (same partial sums, same fold order - by the workgroup of
 *   the graph that arrives last); workspace: gfv_prep_workspace_bytes(B) bytes, 8-byte aligned, its first 4096 bytes (the
 *   arrival counters of up to 1024 graphs: B <= 1024) ZERO before the first launch - every launch leaves them at zero, so one
 *   workspace serves batches of any size one after the other; one workspace per stream that may run this concurrently.
 *   x_raw != NULL: also copies the rows x[:, 0:12] -> x_raw [N,12] (a caller that normalises x in place needs the raw rows
 *   for the edge features).  mean_std != NULL: also derives the Normalizer's (mean[9], std[9]) from acc_count / acc_sum /
 *   acc_sq WITHOUT accumulating (= gfv_normalizer_update(accumulate = 0)); an accumulating step calls gfv_normalizer_update first.
 * gfv_prep_apply: node i < N: uv_old[i] = x_raw[i, 0:2] / uvp_dim[batch[i]], x_out[i] = the normalised row (gfv_node_prep's
 *   arithmetic); edge e < E: out16 / out15 = gfv_edge_attr's relative features of the NORMALISED end-node rows, formed from the
 *   raw rows with the same expressions (bit-identical to gfv_node_prep followed by gfv_edge_attr).  x_raw and x_out are
 *   [N,12] contiguous and must not alias. */
size_t gfv_prep_workspace_bytes(int32_t B);
int gfv_prep_stats(const float* x, int32_t ldx, const int32_t* gnode_ptr, int32_t B, float* stats, void* workspace, float* x_raw,
                   const float* acc_count, const float* acc_sum, const float* acc_sq, float* mean_std, void* stream);
int gfv_prep_apply(const float* x_raw, float* x_out, const int32_t* batch, const float* stats, const float* uvp_dim,
                   const float* mean_std, int32_t norm_global, float* uv_old, int32_t N, const float* pos, const int32_t* es,
                   const int32_t* er, float* out16, float* out15, int32_t E, void* stream);
/* Fused Adam on the flat buffers (torch.optim.Adam defaults; pre_train_Adam.py:115,189-191).  Step counter and
 * hyper-parameters are DEVICE resident so that a captured hipGraph follows learning-rate changes:
 *   state[16]: [0] t = completed steps; [1..2] 1 - beta1^(t+1) as a (hi, lo) float pair and [3] sqrt(1 - beta2^(t+1)): the bias
 *              corrections of the NEXT step, formed in double as torch's host code does; [4] arrival counter (int32, 0 between
 *              launches); [5] 1 - beta1, [6] 1 - beta2 rounded from double (torch: `value = 1 - beta2`); [8..11] the running
 *              powers beta^(t+1) and [12..15] the betas as (hi, lo) pairs.  gfv_adam_state_init writes all of it for a given t and
 *              the betas in DOUBLE (once, and again after a checkpoint load or a change of the betas); every gfv_adam_step_dev
 *              launch then applies it with the lr of hyper[0] as it is at that moment and - its last workgroup to finish -
 *              advances t and the powers by one multiplication (ABI 3: ONE launch per step; ABI 2 had state[4] and a tick
 *              launch in front, gfv_adam_tick_dev / gfv_adam_update_dev: removed)
 *   hyper[8] = {lr, beta1, beta2, eps, grad_scale (1 / world size), w_cont, w_mom, w_press}  (beta1 / beta2 here: the fp32 factors
 *              of the moment decay, as torch's fp32 kernels take them)
 * The same launch publishes the status word once gfv_status_mirror has been called.
 *
 * The five entries gfv_adam_step_dev, _guarded_dev, _accum_dev, _ema_dev and _groups_dev (below) share one launcher: each refuses
 * what its own contract says, the rest - grid, the e / p overlap refusal, the status word - is common.  Which kernel runs follows
 * from the pointers given: groups -> the grouped kernel <guard, accum, e>; else e -> the averaging kernel <guard, accum>; else
 * the plain kernel <guard, accum>, each template flag being "this pointer is not NULL".  So a form reached through a wider entry
 * with its optional pointers NULL runs the same element statements as the narrower entry (the launch sequence). */
int gfv_adam_state_init(float* state, double beta1, double beta2, float steps_done, void* stream);
int gfv_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, const float* hyper,
                      void* stream);
/* Training guard: clip by global norm and leave bad steps out, decided on the device - no host decision, so recorded
 * launch lists and captured graphs keep replaying.  Two launches in place of gfv_adam_step_dev:
 *
 * gfv_grad_guard_dev: ONE launch.  norm = sqrt(sum over the segments of (g[i] * hyper[4])^2): `segs` is a DEVICE table of n_seg
 *   (offset, count) int64 pairs into g - the elements torch would see; nothing outside a segment is read (alignment padding,
 *   slots of parameters without a gradient may hold anything, NaN included).  n_elems = the sum of the counts (it sizes the
 *   grid).  The sum is accumulated in double in a fixed order (no floating-point atomics: same inputs, same bits), each workgroup
 *   leaves one partial in `workspace` and the one that arrives last adds them in index order and writes the decision:
 *   guard[8], 32-bit words (float unless marked):
 *     [0] max_norm            host-written; read when GFV_GUARD_CLIP is set
 *     [1] policy   (int32)    host-written: OR of GFV_GUARD_CLIP | GFV_GUARD_SKIP_NONFINITE | GFV_GUARD_SKIP_FLAG
 *     [2] norm                of the last launch, rounded once from double
 *     [3] coef                fp32 max_norm / (norm + 1e-6f) where that is below 1 or NaN, else exactly 1.0f (clip_grad_norm_'s
 *                             formula); exactly 1.0f without GFV_GUARD_CLIP
 *     [4] decision (int32)    0 = applied as it is; GFV_GUARD_CLIP = applied with coef < 1; GFV_GUARD_SKIP_NONFINITE (the norm is
 *                             inf or NaN and the policy bit is set) and / or GFV_GUARD_SKIP_FLAG (the device status word is
 *                             non-zero and the policy bit is set; the word is read, not cleared) = no step
 *     [5] [6] [7]  (int32)    running counts of launches whose decision carried GFV_GUARD_CLIP, .._SKIP_NONFINITE, .._SKIP_FLAG
 *   workspace: gfv_grad_guard_workspace_bytes() bytes, 8-byte aligned, ZEROED once by the caller (its first word is the arrival
 *   counter, left zero by every launch); one workspace per stream of guard launches.
 * gfv_adam_step_guarded_dev: gfv_adam_step_dev with gi = (g[i] * grad_scale) * guard[3]; with a skip bit in guard[4] it writes
 *   nothing to p, m, v and does not advance state[0] or the running powers (the arrival counter is still reset and the status
 *   word still published).  With coef == 1.0f and no skip its results are those of gfv_adam_step_dev bit for bit.
 * Both return GFV_ERR_ARG (nothing launched) on a NULL pointer, n / n_seg / n_elems < 1 or a misaligned workspace. */
enum { GFV_GUARD_CLIP = 1, GFV_GUARD_SKIP_NONFINITE = 2, GFV_GUARD_SKIP_FLAG = 4 };
size_t gfv_grad_guard_workspace_bytes(void);
int gfv_grad_guard_dev(const float* g, const int64_t* segs, int32_t n_seg, int64_t n_elems, const float* hyper, float* guard,
                       void* workspace, void* stream);
int gfv_adam_step_guarded_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, const float* hyper,
                              const float* guard, void* stream);
/* Gradient accumulation: k micro-batches, one optimiser step.  Three launches in place of the one or two above,
 * the same three on every micro-step - which of them does what is decided on the device, so ONE recorded list or captured
 * graph per batch signature serves all phases.
 *
 * gfv_grad_accum_dev: ONE launch over g[0, n) (n = the whole flat gradient, alignment padding included: harmless, as for Adam).
 *   acc: a second buffer of n floats; B >= 1: the graph count of this micro-batch; loss: the step's device scalar.
 *   accum[8], 32-bit words:
 *     [0] steps     (int32)   k, host-written
 *     [1] micro     (int32)   micro-steps taken in the open accumulation, 0 .. k - 1
 *     [2] graphs    (int32)   graphs summed so far
 *     [3] apply     (int32)   1 if this launch closed an accumulation, else 0
 *     [4] loss_sum            sum of B_i * loss_i of the open accumulation (0 after a close)
 *     [5] loss_mean           loss_sum / graphs of the last closed accumulation
 *     [6] closed    (int32)   running count of closed accumulations
 *     [7]           (int32)   arrival counter, zero between launches
 *   The caller zeroes the record once and writes [0]; to drop an open accumulation it zeroes [1], [2] and [4].
 *   first  (micro == 0):         acc[i] = B * g[i]; acc is NOT read (what an abandoned accumulation left there cannot leak)
 *   middle:                      acc[i] = acc[i] + B * g[i]
 *   last   (micro == steps - 1): g[i] = (acc[i] + B * g[i]) / (graphs + B), the mean over all graphs, written into g for the
 *                                unchanged norm / Adam arithmetic behind it; acc is not written.  (steps == 1: g = B * g / B.)
 *   fp32, product and sum rounded separately.  Every workgroup reads the record before anything in it is written; the one that
 *   arrives last (relaxed integer counter [7], no fence, no floating-point atomics: same inputs, same bits) writes [1] .. [4] and,
 *   on a close, [5], [6], micro = graphs = 0.  16-byte accesses where g and acc are 16-byte aligned, by element otherwise and
 *   for the n % 4 tail.
 * gfv_grad_guard_accum_dev: gfv_grad_guard_dev that, with accum[3] == 0 (a hold micro-step), leaves guard[2..7] untouched; with
 *   accum[3] == 1 its results are those of gfv_grad_guard_dev bit for bit.
 * gfv_adam_step_accum_dev: gfv_adam_step_dev (guard == NULL) or gfv_adam_step_guarded_dev (guard given) that, with accum[3] == 0,
 *   writes nothing to p, m, v and does not advance state[0] or the running powers (arrival counter reset, status word
 *   published, as a skipped step); with accum[3] == 1 the results of those entry points bit for bit.
 * All three return GFV_ERR_ARG (nothing launched) on a NULL pointer (the optional guard apart), n < 0 (accumulate) or n < 1
 * (Adam), B < 1, and what gfv_grad_guard_dev refuses. */
int gfv_grad_accum_dev(float* g, float* acc, int64_t n, int32_t B, const float* loss, float* accum, void* stream);
int gfv_grad_guard_accum_dev(const float* g, const int64_t* segs, int32_t n_seg, int64_t n_elems, const float* hyper, float* guard,
                             void* workspace, const float* accum, void* stream);
int gfv_adam_step_accum_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, const float* hyper,
                            const float* guard, const float* accum, void* stream);
/* Averaged weights: an exponential moving average e of the parameters, advanced inside the Adam launch with the new
 * parameter value still in its register - one more stream (read e, write e: 36 bytes per element instead of 28), no launch.
 *   ema[8], 32-bit words:
 *     [0] decay              host-written (through gfv_ema_init), in [0, 1)
 *     [1] warmup   (int32)   0 or 1, host-written (through gfv_ema_init)
 *     [2] updates  (int32)   number of updates applied to e so far; after gfv_ema_init only the device advances it
 *     [3] w                  weight of the NEXT update: 1 - d_eff, with d_eff = decay (warmup 0) or
 *                            min(decay, (1 + updates) / (10 + updates)) (warmup 1: the average follows a young run closely and
 *                            reaches `decay` at updates = (10 decay - 1) / (1 - decay)); fp32: the quotient, the minimum and the
 *                            difference each rounded once
 *     [4..7]                 zero
 * gfv_ema_init: ONE thread writes all eight words for the given decay, warmup and update count - the formula of w exists in one
 *   place on the device, this launch and the Adam launch below call it.  GFV_ERR_ARG (nothing launched) on a NULL record, a decay
 *   that is NaN or outside [0, 1), a warmup other than 0 or 1, updates < 0.
 * gfv_adam_step_ema_dev: gfv_adam_step_dev (guard == NULL, accum == NULL), gfv_adam_step_guarded_dev (guard given),
 *   gfv_adam_step_accum_dev (accum given, guard optional) - the same template, p, m, v and state bit for bit what those entry
 *   points leave - that also does, per element and with p_new the value it has just stored to p[i],
 *       e[i] = fmaf(w, p_new - e[i], e[i])        (fp32; the difference rounded once, product and sum rounded together)
 *   with w = ema[3] as every thread read it before its loop.  e: n floats that do not overlap p[0, n).  The workgroup that arrives
 *   last at state[4] (the Adam launch's own relaxed arrival counter: no fence, no second counter) then does updates += 1 and
 *   writes the next w.  A step that is not applied - a skip bit in guard[4], accum[3] == 0 - writes neither e nor ema[2], ema[3].
 *   GFV_ERR_ARG (nothing launched) on a NULL pointer (guard and accum apart), n < 1, or e overlapping p (e == p included). */
int gfv_ema_init(float* ema, float decay, int32_t warmup, int32_t updates, void* stream);
int gfv_adam_step_ema_dev(float* p, const float* g, float* m, float* v, float* e, int64_t n, float* state, const float* hyper,
                          const float* guard, const float* accum, float* ema, void* stream);
/* Parameter groups: the Adam launch with a learning rate, a weight decay and a "leave this alone" per GROUP of
 * parameter tensors - torch.optim.Adam / AdamW with param_groups - in the same single launch.  Everything that varies lies in two
 * device tables, so a recorded list or a captured graph follows a change of value as it follows hyper[0]:
 *   run table   one run per parameter tensor of the flat layout, in layout order.  run_start: n_runs + 1 int64, ascending,
 *               run_start[0] = 0, run_start[n_runs] = n (a tensor's alignment padding belongs to its run); run_group: n_runs int32,
 *               the row of each run in the group table, 0 .. GFV_MAX_PARAM_GROUPS (values outside are clamped).  n_runs is at most
 *               GFV_MAX_PARAM_RUNS (the run starts are staged in LDS) and fixed for the life of the owner; membership changes
 *               by rewriting run_group in place.
 *   groups      (GFV_MAX_PARAM_GROUPS + 2) * 8 32-bit words.  Row 0 is the header {n_groups (int32), decoupled (int32), 0 ...}:
 *               decoupled != 0 is AdamW's decay, 0 is Adam's L2 term - one flag of the optimiser, not of a group.  Row 1 + k is
 *               group k: {lr, weight_decay, flags (int32: GFV_GROUP_FROZEN), 0 ...}.  The last row (k = GFV_MAX_PARAM_GROUPS) is
 *               reserved: always frozen, whatever it holds - the group of every parameter without a gradient.
 * Per element of a live run, with lr and wd of its group (hyper[0] is not read):
 *       gi = g[i] * grad_scale (* guard[3] with a guard)         - first, as clip_grad_norm_ comes before step()
 *       L2 (wd != 0):        gi = gi + wd * p[i]
 *       decoupled (wd != 0): p[i] <- p[i] * (float)(1 - (double)lr * (double)wd)
 *       then the statements of gfv_adam_step_dev with step_size = (float)((double)lr / bc1)
 *   betas, eps, the step count and the bias corrections stay shared (state[16], hyper[1..4]).  An element of a frozen run is neither
 *   read nor written: p, m, v and e keep their bits.  A group unfrozen after k steps continues with the SHARED count k + 1 and the
 *   moments it has (zero if it never moved) - torch would start its bias correction at 1.
 * guard, accum, e + ema: each NULL or given, with the meaning and the skip rules of gfv_adam_step_ema_dev (e and ema together).  With
 * one live group, weight_decay 0, the results are those of the entry point of the same form bit for bit.  A thread finds its run
 * by bisection over the run starts (staged in LDS), once per grid sweep and only when its element left the run.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer (guard, accum, e / ema apart), n < 1, n_runs < 1 or > GFV_MAX_PARAM_RUNS,
 * e without ema or ema without e,
 * e overlapping p.  The tables are not validated: the caller builds them (gfv/groups.py). */
#define GFV_MAX_PARAM_GROUPS 32
#define GFV_MAX_PARAM_RUNS 1024
enum { GFV_GROUP_FROZEN = 1 };
int gfv_adam_step_groups_dev(float* p, const float* g, float* m, float* v, float* e, int64_t n, float* state, const float* hyper,
                             const float* guard, const float* accum, float* ema, const int64_t* run_start,
                             const int32_t* run_group, int32_t n_runs, const float* groups, void* stream);
int gfv_train_loss(const float* losses, int32_t B, float w_cont, float w_mom, float w_press, float* loss, float* gloss,
                   void* stream);
/* same, weights read from the device: hyper[5..7] = {w_cont, w_mom, w_press} of the buffer gfv_adam_step_dev takes */
int gfv_train_loss_dev(const float* losses, int32_t B, const float* hyper, float* loss, float* gloss, void* stream);

/* Round 6 - the finite-volume section with fewer launches (FVscheme.py:145-262 and its adjoint; the stand-alone entry points
 * above stay what the operator modules use and what these are tested against, bit for bit).  The mesh tables of a batch in one
 * struct (all device pointers, the tables of gfv_plan_create / gfv/plan.py): */
typedef struct {
  int32_t N, E, C, B;
  int32_t terms;        /* Taylor terms of the WLSQ order: 2 / 5 / 9 / 14 */
  int32_t mode;         /* integrator: 0 explicit, 1 implicit, 2 imex (gfv_phi_fwd) */
  int32_t smooth;       /* gfv_cell_to_node's `smooth` bits */
  int32_t reserved;
  const int32_t* node_type; const int32_t* batch; const int32_t* ftype; const int32_t* cbatch; const int32_t* gcell_ptr;
  const float* pos; const float* fpos; const float* y; const float* centroid; const float* area;
  const float* theta; const float* sigma; const float* uvp_dim; const float* dt;
  const int32_t* crow; const int32_t* kcell; const float* kS;            /* cell <- (face, node) incidences */
  const int32_t* frow; const int32_t* fk;                                /* face <- incidences */
  const int32_t* nfrow; const int32_t* nfcol2;                           /* node <- faces (2 * face + side) */
  const int32_t* nrow; const int32_t* ncell;                             /* node <- incidences */
  const float* An; const float* rn;                                      /* WLSQ moment matrices as stored + row norms */
  const int32_t* xo_rowptr; const int32_t* xo_in; const float* xo_B; const float* sumB;   /* stencil in sender order */
} gfv_fvm_mesh_t;
/* forward tail: gfv_graph_loss + gfv_train_loss_dev (hyper != NULL; its last-arriving workgroup) + gfv_cell_to_node (uvp_node !=
 * NULL) as ONE launch.  counter: one int32 of the caller's, zero before the first launch (the launch leaves it zero).
 * sums [B,4] (the squared residual norms the backward reads) may be NULL in a forward-only step. */
int gfv_fvm_fwd_tail(const gfv_fvm_mesh_t* mesh, const float* cres, const float* phic, const float* phi, float* sums, float* losses,
                     float* uvp_node, const float* hyper, float* loss, float* gloss, int32_t* counter, void* stream);
/* backward of the conserved form from the loss gradients to the gradient of the decoder output, THREE launches (was six:
 * gfv_fvm_bwd_ex's cell / face / node kernels, gfv_wlsq_bwd_ex's solve / gather, gfv_phi_bwd): per face (the cell factors formed on
 * the fly); per (node, channel) the node adjoint + its transposed WLSQ solve; per (node, channel) the stencil gather + the
 * decoder-output adjoint.  Workspaces: gFf_ws [E,16], gphi_ws [N,8], grhs_ws [N,8,terms].  Same sums in the same order as the six. */
int gfv_fvm_bwd_fused(const gfv_fvm_mesh_t* mesh, const float* cres, const float* sums, const float* gloss, const float* Ff,
                      const float* dec, float* gFf_ws, float* gphi_ws, float* grhs_ws, float* gdec, void* stream);

/* k-hop reconstruction stencil of a mesh on the device (per-mesh preprocessing; parse_to_h5.py:228-254,
 * Load_mesh.py:421-521): the unordered node pairs (i < j) with j within k edges of i, as np.unique(axis=1) orders them
 * (by i, then j).  face0 / face1 [F]: the end nodes of every face (int64, as the mesh files hold them; duplicates allowed).
 *   gfv_khop_count builds the CSR adjacency and counts; the number of pairs is then ws[4 (N + 1) - 1] (device memory:
 *   read it back, allocate out0 / out1 [pairs] int64), ws[4 (N + 1)] != 0 says a neighbourhood exceeded 512 nodes (error);
 *   gfv_khop_fill writes the pairs.  ws: gfv_khop_workspace_ints(N, F) int32, untouched between the two calls. */
size_t gfv_khop_workspace_ints(int32_t N, int32_t F);
int gfv_khop_count(const int64_t* face0, const int64_t* face1, int32_t F, int32_t N, int32_t k, int32_t* ws, void* stream);
int gfv_khop_fill(int32_t N, int32_t k, const int32_t* ws, int64_t* out0, int64_t* out1, void* stream);

/* WLSQ moment matrices of a mesh on the device (per-mesh preprocessing; Load_mesh.py:247-272 ->
 * FVgrad.py:183-232 -> FVorder.py:7-86), float64: for node i and its directed stencil entries k in CSR order
 * (rowptr [N+1], outn [S] = the other node of entry k, entry [S] = the entry's position in the caller's edge order):
 *   d = pos[outn[k]] - pos[i], t = the `terms` (2 / 5 / 9 / 14) Taylor monomials of d, w = 1 / |d|,
 *   A[i] (+)= w t t^T  [N, terms, terms],   B[entry[k]] = w t  [S, terms]. */
int gfv_wlsq_moments(const double* pos, const int32_t* rowptr, const int32_t* outn, const int32_t* entry, double* A, double* B,
                     int32_t N, int32_t terms, void* stream);

/* Stand-alone 2nd-order interpolation (FVInterpolation.py `Interplot`: node_to_cell_2nd_order :36-109,
 * node_to_face_2nd_order :111-185, cell_to_node_2nd_order :218-265), any channel count C:
 *   out[r, c] = sum_{k in row r} w_k (phi[col[k], c] + (tgtpos[r] - srcpos[col[k]]) . grad[col[k], c, 0:2]) / W_r
 * mode 0: w = 1, W = max(entries, 1) (mean / average); mode 1: w = 1 / |tgtpos[r] - srcpos[col[k]]|, W = sum w
 * (inverse-distance weights).  grad may be NULL.  wsum [R] receives W (the adjoint needs it).  The adjoint takes the
 * transposed incidence: for source s the forward rows trow[s] .. trow[s+1]-1 of tidx that read it; ggrad may be NULL. */
int gfv_interp2_fwd(const float* phi, const float* grad, const float* srcpos, const float* tgtpos, const int32_t* rowptr,
                    const int32_t* col, int32_t mode, float* out, float* wsum, int32_t R, int32_t C, void* stream);
int gfv_interp2_bwd(const float* gout, const float* wsum, const float* srcpos, const float* tgtpos, const int32_t* trow,
                    const int32_t* tidx, int32_t mode, float* gphi, float* ggrad, int32_t S, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optional per-launch HIP-event timing of the main kernels on their own stream (bench.py roofline leg).
 * kind: 1 row-tile chain, 2 weight gradient, 3 segmented reduce.  out = {launches, total ms, algorithmic flops,
 * algorithmic bytes} summed since the last reset.  Off by default.
 * ---------------------------------------------------------------------------------------------------------- */
int gfv_profile_enable(int on);
int gfv_profile_collect(int kind, double* out);
int gfv_profile_reset(void);
/* kinds: 1 row-tile chain (LDS form), 2 weight gradient, 3 segmented reduce, 4 Transolver slice kernels, 5 finite-volume
 * kernels, 6 input preparation / loss / Adam, 7-10 register-resident chain instantiations, 11 deterministic second-stage
 * reductions, 12 per-step weight images and transposed copies, 13 chain launches with segmented-sum segments, 14 / 15 the
 * column-owner backward (fused weight gradients) / forward family, 16 single-layer launches on the lean kernel.  Sizes an entry point cannot see from its arguments
 * (directed stencil entries S, (cell, face) incidences Sigma) are given here so the finite-volume kernels can be priced. */
int gfv_profile_set_sizes(double stencil_entries, double incidences);

/* ------------------------------------------------------------------------------------------------------------
 * Mesh plan handle: every index table the hot-path kernels walk, built on the device from the
 * reference's own int64 index tensors of one (batched) mesh - what gfv/plan.py builds with torch ops, for callers that
 * have no Python.  The handle owns its tables (device memory) until gfv_plan_destroy; gfv_plan_create synchronises the
 * stream once (it validates every index against its range: GFV_ERR_ARG when one is outside) - it is per-batch set-up,
 * not part of the per-step path.  Stable sorts: inside every CSR row the entries keep the order of the reference's
 * index tensors (the summation order of torch_scatter / index_add).
 *
 * desc (all pointers device memory, int64 as the reference stores them):
 *   edge_index   [2, n_faces]          graph_node.edge_index = face|face_node            (blocks.py:24-31)
 *   cells_node / cells_face / cells_index [n_incidences]  graph_node.face / graph_edge.face / graph_cell.face
 *                                                                                         (FVscheme.py:60-120)
 *   face_node_x  [2, n_stencil_pairs], support_edge [2, n_support_pairs]                  (FVgrad.py:264-271)
 * tables (int32 unless noted; n = rows):
 *   ES, ER [E]                       senders / receivers
 *   N_ROWPTR [N+1], N_COL_NODE, N_COL_EDGE2 [2E], INV_DEG [N] (float)   two-way adjacency by receiving node; the other
 *                                    end of every entry, its slot in the [E, 2] edge message, 1 / max(degree, 1)
 *   S_ROWPTR [N+1], S_COL [E]; R_ROWPTR [N+1], R_COL [E]                edges by sender / by receiver
 *   X_ROWPTR [N+1], X_OUT [S], X_ORDER [S]     directed stencil [fx, fx.flip(0), support] by RECEIVING node: sending
 *                                    node of every entry and its position in the directed list (the caller permutes the
 *                                    moment vectors B by it);  XO_ROWPTR, XO_IN, XO_ORDER: the same by SENDING node
 *   CROW [C+1], K_ORDER, KFACE, KNODE, KCELL [Sigma]   incidences by cell; FROW [E+1], FK [Sigma] by face (entries are
 *                                    positions in the by-cell order); NROW [N+1], NCELL [Sigma] by node
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct gfv_plan gfv_plan_t;
typedef struct {
  int64_t n_nodes, n_faces, n_cells, n_incidences, n_stencil_pairs, n_support_pairs;
  const int64_t* edge_index;
  const int64_t* cells_node;
  const int64_t* cells_face;
  const int64_t* cells_index;
  const int64_t* face_node_x;
  const int64_t* support_edge;
} gfv_plan_desc_t;
enum {
  GFV_PLAN_ES = 0, GFV_PLAN_ER, GFV_PLAN_N_ROWPTR, GFV_PLAN_N_COL_NODE, GFV_PLAN_N_COL_EDGE2, GFV_PLAN_INV_DEG,
  GFV_PLAN_S_ROWPTR, GFV_PLAN_S_COL, GFV_PLAN_R_ROWPTR, GFV_PLAN_R_COL,
  GFV_PLAN_X_ROWPTR, GFV_PLAN_X_OUT, GFV_PLAN_X_ORDER, GFV_PLAN_XO_ROWPTR, GFV_PLAN_XO_IN, GFV_PLAN_XO_ORDER,
  GFV_PLAN_CROW, GFV_PLAN_K_ORDER, GFV_PLAN_KFACE, GFV_PLAN_KNODE, GFV_PLAN_KCELL, GFV_PLAN_FROW, GFV_PLAN_FK,
  GFV_PLAN_NROW, GFV_PLAN_NCELL, GFV_PLAN_TABLE_COUNT
};
int gfv_plan_create(const gfv_plan_desc_t* desc, gfv_plan_t** plan, void* stream);
int gfv_plan_destroy(gfv_plan_t* plan);                 /* NULL is accepted */
/* device pointer and element count of one table (valid until gfv_plan_destroy) */
int gfv_plan_table(const gfv_plan_t* plan, int32_t which, const void** ptr, int64_t* count);
/* sizes5 = {N, E, C, Sigma, S = 2 n_stencil_pairs + n_support_pairs} */
int gfv_plan_sizes(const gfv_plan_t* plan, int64_t* sizes5);

/* ------------------------------------------------------------------------------------------------------------
 * The row-local Linear chains of a Transolver block, one launch each (round 5; split-fp16 product forms only: GFV_ERR_ARG under
 * gfv_set_f16split(0), where the caller issues the three gfv_rowtile_chain launches instead).  All arrays row-major fp32 with
 * row stride = width, 16-byte aligned; img_* = split-fp16 images (gfv_weight_images, built with `wmax`) of the named weights.
 *   forward:   fx1 = out_x W_out^T + b_out + fx_in;   z = LayerNorm(fx1; gamma, beta) W_pre^T + b_pre   [M,256];
 *              out = gelu(z) W_post^T + b_post + fx1          (GraphTransolver.py:93-95,163-169)
 *   backward:  g = g_out (+ g_add) (-> g_sum);  g_z = (g W_post) * gelu'(z);  g_fx1 = LayerNorm-backward(g_z W_pre; fx1, gamma) + g;
 *              g_out_x = g_fx1 W_out;  ln_partial[tile, 0:128 | 128:256] = per-tile (dgamma, dbeta) sums - gfv_trans_mlp_ln_rows(M)
 *              rows (one per 64 rows; one per 32 where the small-tile form of csrc/ctrans.hip takes the launch: provide
 *              gfv_rowtile_ln_rows(M)); sum them with gfv_reduce_multi;  gscale[row / 16] = the 16-row-group scales of g
 *              (gfv_dw_tile_t.gscale).
 *   The backward takes the images of the TRANSPOSED weights: img_post_t of W_post^T [256,128], img_pre_t of W_pre^T [128,256],
 *   img_out_t of W_out^T [128,128].  The weight gradients stay with gfv_dw_multi (they read g / z, g_z / fx1, g_fx1 / out_x).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
  const float* x;        /* out_x [M,128] */
  const float* res;      /* fx_in [M,128] */
  const void* img_out;   /* to_out.0.weight [128,128] */
  const void* img_pre;   /* mlp.linear_pre.0.weight [256,128] */
  const void* img_post;  /* mlp.linear_post.weight [128,256] */
  const float* b_out;    /* [128] or NULL */
  const float* b_pre;    /* [256] or NULL */
  const float* b_post;   /* [128] or NULL */
  const float* gamma;    /* ln_2 [128] */
  const float* beta;
  const float* wmax;
  float* fx1;            /* [M,128] out (saved for the backward) */
  float* z;              /* [M,256] out (saved); fx1 == z == NULL: the forward-only form - neither is stored, `out` has the same bits */
  float* out;            /* [M,128] */
  int32_t M, reserved;
} gfv_trans_mlp_t;
typedef struct {
  const float* g;        /* [M,128] */
  const float* g_add;    /* optional [M,128] */
  float* g_sum;          /* optional [M,128] */
  const float* z;        /* [M,256] */
  const float* fx1;      /* [M,128] */
  const void* img_post_t;
  const void* img_pre_t;
  const void* img_out_t;
  const float* gamma;
  const float* wmax;
  float* g_z;            /* [M,256] out */
  float* g_fx1;          /* [M,128] out */
  float* g_out_x;        /* [M,128] out */
  float* ln_partial;     /* optional [gfv_rowtile_ln_rows(M), 256] (PROVIDE one row per 32 rows; gfv_trans_mlp_ln_rows(M) of them are filled) */
  float* gscale;         /* optional [ceil(M / 128) * 8] */
  int32_t M, reserved;
} gfv_trans_mlp_bwd_t;
int gfv_trans_mlp_fwd(const gfv_trans_mlp_t* args, void* stream);
int gfv_trans_mlp_bwd(const gfv_trans_mlp_bwd_t* args, void* stream);
int gfv_trans_mlp_ln_rows(int32_t M);   /* rows of ln_partial a gfv_trans_mlp_bwd launch over M rows fills (the calling process's switches) */

/* ------------------------------------------------------------------------------------------------------------
 * Native command list (round 5).  Between gfv_record_begin and gfv_record_end every kernel launch the CALLING THREAD issues
 * through this library is executed as usual AND noted - kernel, grid, block, dynamic LDS, stream, arguments by value.
 * gfv_record_replay(handle, first, last) issues the noted launches [first, last) again, on the streams they were recorded on,
 * with no host work but the launches themselves.  What makes a replay valid is the caller's business: the device buffers the
 * recorded arguments point to must still be the step's buffers (gfv/cmdlist.py records inside a private torch memory pool), and
 * host-side decisions (shapes, kernel families, product form) are frozen at record time.  gfv_stream_wait(waiter, waited) is
 * the stream-to-stream edge of such a list: `waiter` waits for everything submitted to `waited` so far (recorded like a launch).
 * gfv_record_count: launches noted so far by the calling thread's open recording (-1: none open).  Replaces, for the replayed
 * step, the per-launch Python / ctypes / argument-check path (the reference pays the same per-op host cost in PyTorch eager:
 * pre_train_Adam.py:158-191).
 * ---------------------------------------------------------------------------------------------------------- */
int gfv_record_begin(void);
int gfv_record_count(void);
int64_t gfv_record_end(void);                 /* -> handle (> 0), 0 if no recording was open */
int gfv_record_length(int64_t handle);
int gfv_record_replay(int64_t handle, int32_t first, int32_t last);
int gfv_record_free(int64_t handle);
int gfv_stream_wait(void* waiter_stream, void* waited_stream);
/* Reorders a recorded list (round 6): every run of commands of other streams than `main_stream` moves behind up to k of the main
 * stream's launches that follow it - never across a command in which the main stream waits, and by at most a third of the distance
 * to it.  A later position only adds ordering (the run's leading wait then covers more of the main stream).  For steps whose main
 * stream runs dry while the host issues a side-stream burst (small meshes).  Returns the number of runs moved, or GFV_ERR_ARG. */
int gfv_record_delay_side(int64_t handle, void* main_stream, int32_t k);

/* ------------------------------------------------------------------------------------------------------------
 * Forward-only rollout (gfv/rollout.py; solve_without_grad_GPU.py:117-173).  The end of a rollout step as ONE launch:
 *   x_backup[:, 0:3] = uvp_node;  x = x_backup          (x_backup, x [N,12], 16-byte aligned)
 *   history[k, b, 0:4] = losses[b];  history[k, b, 4] = || uvp_node - uvp_prev ||_2;  history[k, b, 5] = || uvp_node ||_2
 * over the nodes of graph b, uvp_prev being what x_backup[:, 0:3] held.  k = state[0]; the launch itself stores k + 1 there, so
 * one recorded launch replays for step after step.  state: two int32 of the caller's (step counter, arrival counter), the second
 * zero before the first launch (the launch leaves it zero).  history [K_max, B, 6]; with k >= K_max nothing is written to it and
 * k stays.  chunk_beg / chunk_end [n_chunks]: node ranges that never cross a graph, gchunk_ptr [B + 1] the chunk range of each
 * graph (the plan's slice chunks); partial_ws: 2 * n_chunks doubles.  Sums in a fixed order (double partial sums per chunk, folded
 * per graph by the workgroup that arrives last): no floating-point atomics, results identical run to run.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer or a size < 1.
 * ---------------------------------------------------------------------------------------------------------- */
int gfv_rollout_advance(const float* uvp_node, float* x_backup, float* x, int32_t N, const int32_t* chunk_beg,
                        const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, const float* losses,
                        double* partial_ws, float* history, int32_t K_max, int32_t* state, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Sweep (gfv/sweep.py: a trained model run over the entries of a device pool, slot by slot).  The end of a sweep step as ONE
 * launch: gfv_rollout_advance with per-slot state on the device, so that one recorded launch replays for every step of every
 * batch.  Beside what gfv_rollout_advance takes (no history: per-step records are gfv.rollout.Rollout's):
 *   ctl        16 bytes of device memory the host writes between steps: {float tol (negative: never converge), int32 min_steps,
 *              max_steps, patience}
 *   slots      [B, 4] int32: age (steps this entry has taken), streak (consecutive steps with a relative update below tol),
 *              done (0 live, 1 converged, 2 stopped at max_steps), reserved
 *   last       [B, 6] float: the gfv_rollout_advance history row of the slot's last live step
 *   state3     [N, 3] float: what x_backup[:, 0:3] holds after the launch, compact (the source of gfv_pool_payback)
 *   mirror_dev the device address of a pinned, device-mapped int32 array of at least 1 + 2 B words (gfv_sweep_mirror_create):
 *              [0] the step sequence number, [1 + 2 b] done and [2 + 2 b] age of slot b - a hint the host reads without a
 *              synchronisation; whatever it acts on it reads from slots / last after one
 *   state      two int32 (step sequence number, arrival counter), the second zero before the first launch and left zero
 * For slot b = the graph of a chunk (gchunk_ptr), with done[b] AS THE LAUNCH FINDS IT:
 *   live:    x_backup[:, 0:3] = uvp_node; x = x_backup; state3 = uvp_node; then, by the workgroup that arrives last:
 *            age += 1; rel = || uvp_node - uvp_prev ||_2 / || uvp_node ||_2 (fp32 quotient of the two fp32 norms);
 *            streak = rel < tol ? streak + 1 : 0 (a NaN or a zero norm compares false);
 *            done = 1 if streak >= patience && age >= min_steps, else 2 if age >= max_steps; last[b] is written
 *   frozen:  x = x_backup; state3 = x_backup[:, 0:3]; x_backup, slots[b] and last[b] stay as they are
 * done is written only after every workgroup has arrived: a slot's final field is the prediction of the step that latched it,
 * whatever was queued behind it.  Sums in the fixed order of gfv_rollout_advance; no floating-point atomics.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer, a size < 1 or an x_backup / x that is not 16-byte aligned.
 * gfv_sweep_mirror_create: n_words zeroed int32 of pinned, device-mapped host memory -> its host and device addresses;
 * gfv_sweep_mirror_free takes the host address.  GFV_ERR_ARG on n_words < 1 or a NULL pointer.
 * ---------------------------------------------------------------------------------------------------------- */
int gfv_sweep_mirror_create(int32_t n_words, int32_t** host_words, int32_t** dev_words);
int gfv_sweep_mirror_free(int32_t* host_words);
int gfv_sweep_advance(const float* uvp_node, float* x_backup, float* x, int32_t N, const int32_t* chunk_beg,
                      const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, const float* losses,
                      double* partial_ws, const void* ctl, int32_t* slots, float* last, float* state3, int32_t* mirror_dev,
                      int32_t* state, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Time march (gfv/march.py; solve_with_grad_GPU.py:133-209 with the --residual_tolerance / --max_inner_steps of
 * utils/get_param.py:54-55): advance in time only after the inner iterations of a time level have converged, decided on the
 * device.  ONE launch per training step, on the main stream, behind the backward and in front of the optimiser's launches.
 * Beside what gfv_rollout_advance takes (uvp_node, x_backup, x, N, the chunk tables, B, losses, partial_ws):
 *   hyper      the 8 floats of gfv_adam_step_dev; [5], [6], [7] = w_cont, w_mom, w_press are read
 *   march      16 32-bit words of the caller's, zeroed once, then the host-written words set:
 *     [0] max_inner (int32, host)    inner iterations per level at most
 *     [1] min_inner (int32, host)    ... and at least
 *     [2] inner     (int32)          inner iterations taken in the open level
 *     [3] apply     (int32)          1 if this step is a step, 0 if it is held - at the position the Adam, guard and log launches
 *                                    read as accum[3] (gfv_adam_step_accum_dev, gfv_grad_guard_accum_dev, gfv_train_log_append)
 *     [4] tol       (float, host)    relative tolerance on r / r0; negative: never fires
 *     [5] abs_tol   (float, host)    absolute tolerance on r; negative: never fires
 *     [6] level     (int32)          levels completed
 *     [7]           (int32)          arrival counter, zero between launches
 *     [8] target    (int32, host)    levels to complete
 *     [9] done      (int32)          1 once level >= target (or the history is full)
 *     [10] seen     (int32)          launches that found done clear
 *     [11] held     (int32)          launches that found done set
 *     [12] keep     (int32, host)    snapshots kept, 0 .. the argument `keep`
 *     [13..15]                       zero
 *   r0         [B] float: the residual of each graph at the first inner iteration of the open level
 *   history    [max_levels, GFV_MARCH_HEAD + GFV_MARCH_GRAPH * B] 32-bit words, one row per completed level:
 *                head {level, inner iterations taken, flags GFV_MARCH_CONVERGED | GFV_MARCH_CAPPED, seen, 0, 0, 0, 0} (int32),
 *                then per graph 8 floats: the four loss terms (bit copies), r0, r, || uvp_node - uvp_prev ||_2, || uvp_node ||_2
 *   max_inner, min_inner   the values the host has written to march[0] and [1]: the entry point cannot read device memory, so it
 *              checks these; the kernel reads the record's (a recorded launch follows a later host write) and, should they be out
 *              of range there, uses max(max_inner, 1) and min_inner clamped to [1, max_inner]
 *   snap, keep an optional ring [keep, N, 3] float of the last levels' fields (keep == 0: snap may be NULL); the kernel uses
 *              min(march[12], keep) rows of it
 *   mirror_dev optional: the device address of 3 pinned, device-mapped int32 (gfv_sweep_mirror_create) that receive {seen, level,
 *              done} by plain stores - a hint the host reads without a synchronisation
 * The rule, with the record AS THE LAUNCH FINDS IT (every workgroup reads it, r0 and losses before anything is written; the
 * workgroup that arrives last writes it - the discipline of gfv_grad_accum_dev):
 *   done set:     apply = 0; held += 1.  Nothing else changes.
 *   done not set: apply = 1; seen += 1; per graph r = w_press * press + w_cont * cont + w_mom * mom_x + w_mom * mom_y in fp32, the
 *                 statement that forms the argument of the logarithm in gfv_train_loss_dev (one shared inline function);
 *                 inner == 0: r0 = r;  conv = (tol >= 0 && r <= tol * r0) || (abs_tol >= 0 && r <= abs_tol) - the product one fp32
 *                 rounding, a NaN compares false;  k = inner + 1;  latch = (every graph conv && k >= min_inner) || k >= max_inner
 *     no latch:   inner = k.  No row of x_backup, x or uvp_node is read or written.
 *     latch:      x_backup[:, 0:3] = uvp_node; x = x_backup; snap[level % keep] = uvp_node; history row `level` (norms in the
 *                 summation order of gfv_rollout_advance: double partial sums per chunk, folded per graph by the workgroup that
 *                 arrives last, one rounding to fp32; no floating-point atomics); inner = 0; level += 1; done = level >= target.
 *                 With level >= max_levels no row is written and done is set.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer (snap: only with keep > 0; mirror_dev: never), N, n_chunks, B or max_levels
 * < 1, keep < 0, max_inner < 1, min_inner outside [1, max_inner] or an x_backup / x that is not 16-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_MARCH_RECORD 16
#define GFV_MARCH_HEAD 8
#define GFV_MARCH_GRAPH 8
#define GFV_MARCH_CONVERGED 1u
#define GFV_MARCH_CAPPED 2u
int gfv_march_advance(const float* uvp_node, float* x_backup, float* x, int32_t N, const int32_t* chunk_beg,
                      const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, const float* losses,
                      double* partial_ws, const float* hyper, int32_t* march, float* r0, void* history, int32_t max_levels,
                      int32_t max_inner, int32_t min_inner, float* snap, int32_t keep, int32_t* mirror_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The sampling window (gfv/window.py, csrc/gfv_window.h): which fields of a run the launches that sample it from
 * behind its advance launch take - gfv_field_stats_update; gfv_wall_force_grad and gfv_wall_force_sum; gfv_probe_sample;
 * gfv_flow_integrals.
 *   clock      the device address of one int32 that increases whenever a new field has been written: word 0 of
 *              gfv_rollout_advance's state, word [6] `level` of gfv_march_advance's record (the idea of GFV_SCHED_FOLLOW)
 *   rec        GFV_WINDOW_RECORD 32-bit words of the caller's, one record per sampler:
 *     [0] start    (int32, host)    the first clock value to sample
 *     [1] stride   (int32, host)    sampling stride; values < 1 are read as 1
 *     [2] stop     (int32, host)    exclusive end; negative: none
 *     [3] last     (int32)          the clock value the last launch found; -1 after a reset
 *     [4] n        (int32)          samples taken
 *     [5]          (int32)          arrival counter, zero between launches
 *     [6] enabled  (int32, host)    0 pauses sampling
 *     [7]                           zero
 * The rule, with rec and *clock AS THE LAUNCH FINDS THEM (every thread reads them before anything is written; the workgroup that
 * arrives last - of a sampler's last launch - writes the record, so the launches of one sampler decide alike):
 *   c = *clock
 *   take = enabled && c != last && c >= start && (stop < 0 || c < stop) && (c - start) % max(stride, 1) == 0
 *   take false:  nothing of the sampler's state is read or written
 *   take true:   the sampler's own rule, below
 *   then, always:  last = c if it differs;  n += 1 if take;  the counter back to 0
 * So a reset is last = -1, n = 0.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_WINDOW_RECORD 8

/* ------------------------------------------------------------------------------------------------------------
 * Field statistics (gfv/fieldstats.py): the time mean, the variances, the Reynolds shear stress u'v' and the
 * extremes of the node field over a window of a run, kept on the device.  ONE launch behind the launch that has advanced the
 * field (gfv_rollout_advance, gfv_march_advance), on the same stream.
 *   x_backup   [N, 12] float, 16-byte aligned: columns 0:3 of a row are the field (u, v, p); nothing else of a row is used
 *   clock, rec the clock and the window's record (GFV_WINDOW_RECORD, above)
 *   sums       double [GFV_FIELD_STATS_SUMS, N], planar: S1u, S1v, S1p, S2uu, S2vv, S2pp, S2uv
 *   aux        float [GFV_FIELD_STATS_AUX, N], planar: the shift K of u, v, p; the minimum of u, v, p; the maximum of u, v, p
 * The rule: the window's (take false: no row and no element of sums or aux is read or written), and with take true, per row, x
 * the row's three floats:
 *     n == 0:    K = min = max = x; all seven sums are written as +0.0 (so a reset needs no memset)
 *     n > 0:     d = (double)x - (double)K per channel; S1 += d; S2uu += du * du; S2vv += dv * dv; S2pp += dp * dp;
 *                S2uv += du * dv - each product and each sum ONE IEEE double operation, nothing contracted;
 *                min = fminf(min, x); max = fmaxf(max, x) (a NaN sample leaves them; a NaN they hold is replaced)
 * So mean = K + S1 / n, the population variance S2 / n - (S1 / n)^2, cov(u, v) = S2uv / n - (S1u / n)(S1v / n): shifted by the
 * first sample, the sums stay of the size of the fluctuation.  No floating-point atomics and no sum across rows: the same
 * inputs give the same bits, whatever the grid.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer, N < 1 or an x_backup that is not 16-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_FIELD_STATS_RECORD 8 /* = GFV_WINDOW_RECORD */
#define GFV_FIELD_STATS_SUMS 7
#define GFV_FIELD_STATS_AUX 9
int gfv_field_stats_update(const float* x_backup, int32_t N, const int32_t* clock, int32_t* rec, double* sums, float* aux,
                           void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Unsteady boundary data (gfv/timebc.py): the Dirichlet velocity targets and the source coefficient as functions
 * of time, rewritten for the field about to be computed.  ONE launch behind the launch that has advanced the field
 * (gfv_rollout_advance, gfv_march_advance), on the same stream.
 *   clock      the device address of one int32 counting the fields written so far (gfv_field_stats_update's clock)
 *   ctl        GFV_TIME_BC_CTL int32 words of the caller's: [0] offset (host) added to the clock; the rest zero
 *   rec        double [B, 2, GFV_TIME_BC_RECORD], 8-byte aligned: per graph the velocity waveform's record, then the source's:
 *     d[0] kind   GFV_TIME_BC_NONE .. GFV_TIME_BC_TABLE_PERIODIC (a whole number)
 *     CONST:        d[1] value
 *     RAMP_*:       d[1] g0, d[2] g1, d[3] t0, d[4] t1 (t1 > t0)
 *     SINE:         d[1] mean, d[2] amp, d[3] freq, d[4] phase, d[5] start
 *     TABLE*:       d[1] n, 1 .. GFV_TIME_BC_TABLE_MAX points (PERIODIC: at least 2) in the record's slot of `tab`
 *   tab        double [B, 2, 2, GFV_TIME_BC_TABLE_MAX]: per record its times (strictly increasing), then its values; NULL when no
 *              record is a table
 *   dt         float [B];  batch, node_type  int32 [N]
 *   y0, y      float [N, 2], 8-byte aligned, distinct: the base targets (read) and the targets the forward reads (written)
 *   theta0     float [B]: the base source coefficient;  theta5: the address of element (0, 5) of the coefficient table the forward
 *              reads, ld_theta floats per graph
 *   x_backup, x  float [N, 12] or NULL: node-feature column 8 (= 3 + 5) of every row takes the value written to theta5
 *   hist       double [K_max, B, GFV_TIME_BC_HIST] or NULL: row c - 1 = (t, g_v, g_s) per graph, written for 1 <= c <= K_max
 *   type_mask  bit k set: rows of node type k (0 .. 5) take the velocity waveform
 *   channels   bit 0: the velocity channel, bit 1: the source channel; a channel that is off writes nothing (its g is recorded as 1)
 * With c = *clock + 1 + ctl[0] and, per graph b, t = (double)c * (double)dt[b] - every operation below ONE IEEE double operation
 * in the order written, nothing contracted:
 *   CONST         g = value
 *   RAMP_LINEAR   s = min(max((t - t0) / (t1 - t0), 0), 1);  g = g0 + (g1 - g0) * s
 *   RAMP_SMOOTH   s as above;  g = g0 + (g1 - g0) * ((s * s) * (3 - 2 * s))
 *   SINE          g = mean + amp * sin(((2 pi * freq) * max(t - start, 0)) + phase)    (2 pi: the double 6.283185307179586; sin
 *                 is the device library's: within DESIGN.md 5u's measured distance of the correctly rounded value)
 *   TABLE         t <= T[0]: V[0];  t >= T[n-1]: V[n-1];  else with T[k] <= t < T[k+1]:
 *                 g = V[k] + (V[k+1] - V[k]) * ((t - T[k]) / (T[k+1] - T[k]))
 *   TABLE_PERIODIC  m = fmod(t - T[0], T[n-1] - T[0]); m += T[n-1] - T[0] if m < 0;  t = T[0] + m;  then as TABLE
 *   row i of graph b, node_type[i] in the mask, velocity on:   y[i, 0:2] = (float)(g_v * (double)y0[i, 0:2])
 *   every row i of graph b, source on:                         x_backup[i, 8] = x[i, 8] = (float)(g_s * (double)theta0[b])
 *   per graph:                                                 theta5[b * ld_theta] = the same float; the history row
 * Every other element is left as it is.  Nothing written is read: a launch that finds the same clock writes the same bits.
 * GFV_ERR_ARG (nothing launched) on a NULL clock, ctl, rec, dt, batch or node_type, N or B < 1, channels outside 1 .. 3, a
 * type_mask beyond bit 5, the velocity channel without y0 / y (or y0 == y, or either not 8-byte aligned), the source channel
 * without theta0 / theta5 or ld_theta < 1, hist with K_max < 1, or a rec / tab / hist that is not 8-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_TIME_BC_RECORD 8
#define GFV_TIME_BC_CTL 4
#define GFV_TIME_BC_HIST 3
#define GFV_TIME_BC_TABLE_MAX 1024
#define GFV_TIME_BC_NONE 0
#define GFV_TIME_BC_CONST 1
#define GFV_TIME_BC_RAMP_LINEAR 2
#define GFV_TIME_BC_RAMP_SMOOTH 3
#define GFV_TIME_BC_SINE 4
#define GFV_TIME_BC_TABLE 5
#define GFV_TIME_BC_TABLE_PERIODIC 6
int gfv_time_bc_update(const int32_t* clock, const int32_t* ctl, const double* rec, const double* tab, const float* dt,
                       const int32_t* batch, const int32_t* node_type, int32_t N, int32_t B, const float* y0, float* y,
                       const float* theta0, float* theta5, int32_t ld_theta, float* x_backup, float* x, double* hist,
                       int32_t K_max, int32_t type_mask, int32_t channels, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Time differencing of a march (gfv/timescheme.py): the history of a second-order backward difference (BDF2), kept
 * on the device.  The momentum residual's time term is theta0 * (u - u_old) / dt * area and is linear in u_old, so BDF2 is that
 * term with two substitutions: u_old -> u* = u_n + (u_n - u_{n-1}) / 3 and dt -> dt / 1.5, since
 * (u - u*) / (dt / 1.5) = (3 u - 4 u_n + u_{n-1}) / (2 dt).  ONE launch behind whatever has advanced the field
 * (gfv_march_advance, or the two copies of TrainStep.advance_time()), on the same stream, writes u* and the step the
 * finite-volume section then reads (gfv_phi_fwd_ts; the `dt` of gfv_cell_fwd_ex, gfv_fvm_bwd_ex and gfv_fvm_mesh_t).
 *   x_backup   [N, 12] float, 16-byte aligned: columns 0:2 of a row are the velocity (u, v), dimensional
 *   batch      int32 [N]: the graph of a row;  uvp_dim  float [B, 3];  dt  float [B] (read, never written)
 *   clock      the device address of one int32 counting the fields written so far: x_backup holds field *clock, field 0 is the
 *              initial state (word [6] `level` of gfv_march_advance's record, or a word of the caller's own)
 *   rec        GFV_TIME_SCHEME_RECORD int32 words, all written by the host only:
 *     [0] scheme   GFV_TIME_SCHEME_BDF1 or GFV_TIME_SCHEME_BDF2
 *     [1] base     the clock of the oldest field the ring is known to hold
 *     [2], [3]     zero
 *   ring       float [2, N, 2], 8-byte aligned: the velocity columns of the fields seen, one slot per clock parity
 *   ustar      float [N, 2], 8-byte aligned: the dimensionless baseline of the time difference, in the form gfv_prep_apply's
 *              uv_old has
 *   dt_eff     float [B]: the step of the time difference
 * The rule, with rec and *clock AS THE LAUNCH FINDS THEM (every thread reads them before anything is written; the launch
 * writes neither):
 *   c = *clock;  active = (scheme == GFV_TIME_SCHEME_BDF2) && (c > base)
 *   row i < N of graph b = batch[i], channel k in {0, 1}:
 *     cur = x_backup[i, k];  ring[c & 1][i][k] = cur
 *     active:      prev = ring[(c & 1) ^ 1][i][k];  s = cur + (cur - prev) / 3.0f;  ustar[i][k] = s / uvp_dim[3 b + k]
 *     otherwise:   ustar[i][k] = cur / uvp_dim[3 b + k]       (gfv_prep_apply's uv_old: the same operation, the same bits)
 *   t < B:         dt_eff[t] = active ? dt[t] / 1.5f : dt[t]
 * Every operation is ONE IEEE float operation in the order written, nothing contracted.  The launch reads only the ring slot it
 * does not write, and x_backup: a launch that finds the same clock (an inner iteration, a held step of a march) writes the same
 * bits again, and a launch that finds the clock advanced by one overwrites field c - 2 with field c and reads field c - 1 - the
 * whole rotation.  One thread per row, no atomics, no sum across rows, no word written that another workgroup of the launch reads.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer, N < 1, B < 1, an x_backup that is not 16-byte aligned or a ring / ustar that
 * is not 8-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_TIME_SCHEME_RECORD 4
#define GFV_TIME_SCHEME_BDF1 1
#define GFV_TIME_SCHEME_BDF2 2
int gfv_time_scheme_update(const float* x_backup, const int32_t* batch, const float* uvp_dim, const float* dt, int32_t N,
                           int32_t B, const int32_t* clock, const int32_t* rec, float* ring, float* ustar, float* dt_eff,
                           void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Adaptive time step of a march (gfv/timescheme.py StepControl): the step sized to a Courant-number target and the
 * variable-step form of BDF2.  TWO launches in place of gfv_time_scheme_update, behind whatever has advanced the field, on the
 * same stream: gfv_step_control_rate, then gfv_step_control_rows.  `x_backup`, `batch`, `uvp_dim`, `dt`, `clock`, `rec`, `ring`,
 * `ustar` and `dt_eff` are gfv_time_scheme_update's.  New, everything per graph b:
 *   crow int32 [C + 1], knode int32 [crow[C]], kS float [crow[C], 2] (8-byte aligned), area float [C], cbatch int32 [C] ascending:
 *              the (cell, node) incidences of the plan and their face vectors
 *   crec       GFV_STEP_CONTROL_RECORD int32 words: [0] tbase (host): the last clock whose step and time are the host's (dt0, time0);
 *              [1] the arrival counter (zero between launches);  [2], [3] zero
 *   par        GFV_STEP_CONTROL_PARAMS floats (host): courant, grow, shrink, min_factor, max_factor, 0, 0, 0
 *   dt0 float [B], time0 double [B] (host): the step that produced field tbase and its time
 *   rate       uint32 [2, B]: the bits of the Courant rate, one slot per clock parity; both zero before the first launch
 *   dts        float [2, B]: dts[c & 1] the step that produced field c;   times  double [2, B]: times[c & 1] the time of field c
 *   state      float [GFV_STEP_CONTROL_STATE, B]: rows dt_next, omega, courant, rate - of the clock the last launch found
 *   hist_clock int32 [keep], hist float [keep, 2, B] (dt_next, courant), hist_time double [keep, B]: row c % keep
 * The rule, with c = *clock, rec, crec[0] and par AS THE LAUNCH FINDS THEM; every operation ONE IEEE float operation in the order
 * written, nothing contracted, sums over k ascending from +0:
 *   cell j of graph b = cbatch[j], k in crow[j] .. crow[j + 1] - 1, n their number (n = 0: rate_j = 0):
 *     sx = sum_k x_backup[knode[k], 0] / uvp_dim[3 b];  sy likewise with column 1 and uvp_dim[3 b + 1];  mx = sx / n;  my = sy / n
 *     rate_j = (sum_k |mx * kS[k, 0] + my * kS[k, 1]|) / (2 * area[j]);  anything not > 0 (a NaN too) counts as +0
 *   rate[c & 1][b] = max(rate[c & 1][b], max_j rate_j) by integer maxima of the bits (exact in any order);  rate[(c & 1) ^ 1][b] = 0
 *   then, by the workgroup that arrives last, with first = (c <= tbase), active = (scheme == GFV_TIME_SCHEME_BDF2 && c > base):
 *     dt_last = first ? dt0[b] : dts[c & 1][b];   Co = rate * dt_last
 *     fac = Co > 0 ? courant / Co : grow;   fac = min(max(fac, shrink), grow)
 *     dt_next = dt_last * fac;   dt_next = min(max(dt_next, min_factor * dt[b]), max_factor * dt[b]);   omega = dt_next / dt_last
 *     dt_eff[b] = active ? dt_next / ((1 + 2 * omega) / (1 + omega)) : dt_next
 *     time = first ? time0[b] : times[(c & 1) ^ 1][b] + (double)dt_last          (one double addition)
 *     dts[(c + 1) & 1][b] = dt_next;  times[c & 1][b] = time;  state and the history row c % keep as above;  hist_clock = c
 *   gfv_step_control_rows, row i of graph b, channel k, cur and prev as in gfv_time_scheme_update:
 *     active:      q = (1 + 2 * omega) / (omega * omega);  s = cur + (cur - prev) / q;  ustar[i][k] = s / uvp_dim[3 b + k]
 *     otherwise:   ustar[i][k] = cur / uvp_dim[3 b + k];      either way ring[c & 1][i][k] = cur
 * The weights omega^2 / (1 + 2 omega) and (1 + omega) / (1 + 2 omega) are applied as divisions by their reciprocals: at omega = 1
 * the divisors are exactly 3 and 1.5, and the pair writes the bits of gfv_time_scheme_update.  The pair reads no word it writes (the rate slot it adds to takes
 * a maximum: adding the same cells again leaves it), so a pair that finds the clock it found before writes the same bits
 * everywhere, the history row included.  `dt` is never written.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer, C, B, N or keep < 1, an x_backup that is not 16-byte aligned, or a kS, time0,
 * times, hist_time, ring or ustar that is not 8-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_STEP_CONTROL_RECORD 4
#define GFV_STEP_CONTROL_PARAMS 8
#define GFV_STEP_CONTROL_STATE 4
int gfv_step_control_rate(const float* x_backup, const float* uvp_dim, const float* dt, const int32_t* crow, const int32_t* knode,
                          const float* kS, const float* area, const int32_t* cbatch, int32_t C, int32_t B, const int32_t* clock,
                          const int32_t* rec, int32_t* crec, const float* par, const float* dt0, const double* time0,
                          uint32_t* rate, float* dts, double* times, float* state, float* dt_eff, int32_t* hist_clock, float* hist,
                          double* hist_time, int32_t keep, void* stream);
int gfv_step_control_rows(const float* x_backup, const int32_t* batch, const float* uvp_dim, int32_t N, int32_t B,
                          const int32_t* clock, const int32_t* rec, const float* state, float* ring, float* ustar, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Wall forces (gfv/wallforce.py): the pressure force and the viscous force of the fluid on a body and their moments,
 * per graph, for the field a run has just written - the momentum flux the residual itself attributes to the wall faces (P_flux -
 * vis_flux of FVscheme.py:203-229; the convective flux is left out: it is zero on a wall whose velocity has no normal component).
 * TWO launches behind the launch that has advanced the field (gfv_rollout_advance, gfv_march_advance), on the same stream:
 * gfv_wall_force_grad, then gfv_wall_force_sum.  `x_backup` is gfv_field_stats_update's; `clock` and `rec` are the clock and the
 * window's record (GFV_WINDOW_RECORD, above).
 *   uvp_dim float [B, 3];  batch int32 [N];  theta float [B, ld_theta], ld_theta >= 5: columns 3 and 4 are read at every launch
 *   x_rowptr int32 [N + 1], x_out int32 [S], x_B float [S, terms], An float [N, terms * terms], rn float [N, terms]: the WLSQ
 *              stencil of the plan, as gfv_wlsq_fwd_ex takes it;  terms 2 / 5 / 9 / 14
 *   pos float [N, 2], fpos float [E, 2], es, er int32 [E], kS float [Sg, 2]: node and face positions, a face's end nodes, the
 *              surface vector of a (cell, face) incidence - the cell's OUTWARD vector, so on a wall face it points into the body
 *   bnode      int32 [Nb]: the selected faces' end nodes, unique and ascending
 *   wface      int32 [Nf, 4], 16-byte aligned: per selected face (f, k, ja, jb) - the face, its one incidence, the positions of
 *              es[f] and er[f] in bnode; rows ascending in f, hence grouped by graph
 *   wchunk_beg, wchunk_end int32 [n_wchunks], gwchunk_ptr int32 [B + 1]: chunks of at most GFV_WALL_FORCE_CHUNK consecutive rows
 *              of wface that never cross a graph, and each graph's range of chunks (the form of a plan's chunk tables)
 *   origin     float [B, 2] (host): the point the moments are taken about
 *   gb         double [Nb, 3, 2]: the body nodes' gradients (written by the first launch, read by the second)
 *   partial    double [n_wchunks, GFV_WALL_FORCE_SUMS]: workspace
 *   hist       double [keep, B, GFV_WALL_FORCE_SUMS]: (Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv) per graph, row n % keep
 *   hist_clock int32 [keep]: the clock of a row
 * The rule: the window's, each launch with rec and *clock as it finds them (only the last arriver of the second launch writes rec).
 *   take false:  the first launch reads and writes nothing; the second moves no word of partial, hist or hist_clock
 *   take true:
 *     phi_c(i) = x_backup[i, c] / uvp_dim[3 batch[i] + c], c = u, v, p: ONE fp32 division (gfv_step_control_rate's convention)
 *     gb[j, c, 0:2], i = bnode[j]: the arithmetic of gfv_wlsq_fwd_ex - rhs_m = sum_s (double)x_B[s, m] * ((double)phi_c(x_out[s]) -
 *       (double)phi_c(i)) over s = x_rowptr[i] .. x_rowptr[i + 1] - 1 ascending, from +0; rhs_m / (double)rn[i, m]; the matrix
 *       (double)An[i, r, q] * (1 / (double)rn[i, r]); LU with partial pivoting and the solve in double - the first two entries of
 *       the solution, kept in double
 *     per row (f, k, ja, jb) of wface, graph b, s = es[f], r = er[f], S = kS[k], g_s = gb[ja], g_r = gb[jb]; everything below one
 *     IEEE double operation in the order written, nothing contracted, except where fp32 is named:
 *       r_s = fpos[f] - pos[s], r_r = fpos[f] - pos[r]                                  (fp32, as gfv_face_fwd forms them)
 *       v_s = phi_p(s) + (r_s.x * g_s[p][0] + r_s.y * g_s[p][1]);  v_r likewise;  p_f = 0.5 * (v_s + v_r)
 *       Fp = ((theta3 * p_f) * S.x, (theta3 * p_f) * S.y)
 *       G[c][a] = 0.5 * (g_s[c][a] + g_r[c][a]), c = u, v;   Fv[c] = -(theta4 * (G[c][0] * S.x + G[c][1] * S.y))
 *       arm = (double)fpos[f] - (double)origin[b];  Mp = arm.x * Fp.y - arm.y * Fp.x;  Mv likewise
 *     (no wall overwrite of the face velocity: it concerns u, v, which nothing here reads.)  Fp + Fv is the force of the fluid
 *     ON THE WALL.
 *     per chunk: one wave; lane l adds the rows beg + l, beg + l + 64, ... < min(end, Nf) in ascending order from +0.0, the 64
 *     lane sums fold by the xor butterfly 32, 16, ... 1; per graph, by the workgroup that arrives last: lane l adds the chunk
 *     sums c0 + l, c0 + l + 64, ... in ascending order, then the same butterfly (csrc/gfv_reduce.h states the order)
 *     hist[n % keep, b, :] = the graph's six sums (zero for a graph without a face);  hist_clock[n % keep] = c
 * No floating-point atomics and no sum across graphs: the same inputs give the same bits, whatever the grid.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer, Nb, Nf, n_wchunks, B or keep < 1, ld_theta < 5, terms outside the four
 * values, an x_backup or wface that is not 16-byte aligned, or a gb, partial or hist that is not 8-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_WALL_FORCE_RECORD 8 /* = GFV_WINDOW_RECORD */
#define GFV_WALL_FORCE_SUMS 6
#define GFV_WALL_FORCE_CHUNK 64
int gfv_wall_force_grad(const float* x_backup, const float* uvp_dim, const int32_t* batch, const int32_t* x_rowptr,
                        const int32_t* x_out, const float* x_B, const float* An, const float* rn, const int32_t* bnode, int32_t Nb,
                        int32_t terms, const int32_t* clock, const int32_t* rec, double* gb, void* stream);
int gfv_wall_force_sum(const float* x_backup, const float* uvp_dim, const float* theta, int32_t ld_theta, const float* pos,
                       const float* fpos, const float* kS, const int32_t* es, const int32_t* er, const int32_t* wface,
                       const int32_t* wchunk_beg, const int32_t* wchunk_end, const int32_t* gwchunk_ptr, int32_t n_wchunks,
                       int32_t Nf, int32_t B, const float* origin, const double* gb, const int32_t* clock, int32_t* rec,
                       double* partial, double* hist, int32_t* hist_clock, int32_t keep, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Probes (gfv/probes.py): the value and the gradient of (u, v, p) at fixed points of the mesh, for the field a run
 * has just written.  ONE launch behind the launch that has advanced the field (gfv_rollout_advance, gfv_march_advance), on the same
 * stream.  `x_backup`, `uvp_dim` and `batch` are gfv_wall_force_grad's; `clock` and `rec` are the clock and the window's record
 * (GFV_WINDOW_RECORD, above).
 *
 * What a probe is (fixed when the tables are built, on the host, in float64; nothing of it is done by the launch).
 *   units      phi_c(n) = x_backup[n, c] / uvp_dim[3 batch[n] + c], c = u, v, p: ONE fp32 division, then double
 *   location   a probe is a point x (double) and the graph b it lies in.  Over the cells C of graph b (gcell_ptr[b] ..
 *              gcell_ptr[b + 1] - 1), with the incidences k = crow[C] .. crow[C + 1] - 1 of a cell, its outward face vectors kS[k]
 *              and the stored face centres fpos[kface[k]] (fp32 data, every operation in double):
 *                  d(C) = max_k ((x - fpos[kface[k]]) . kS[k]) / |kS[k]|
 *              the signed distance by which x lies outside the cell's farthest face line; d <= 0 exactly inside a CONVEX cell
 *              (cells are taken as convex).  The probe's cell is the cell of least d, the lowest index among equals (a point at
 *              an interior face's stored centre has d = 0 exactly in both neighbours).  outside = d_min / sqrt(area[cell]); a
 *              probe with outside > tolerance is refused, an accepted one is not moved.
 *   value      the cell's vertices are V = knode[crow[C] .. crow[C + 1] - 1], k of them; g_v[c] is the WLSQ gradient of phi_c at
 *              vertex v - the first two entries of the solution of the row-normalised system of gfv_wall_force_grad, any of the
 *              four orders.  The scheme's own second-order reconstruction (node value plus gradient times offset, the ends
 *              averaged, as gfv_face_fwd forms a face value from two ends), over the k vertices with EQUAL weights:
 *                  value_c(x)    = (1 / k) sum_v ( phi_c(v) + g_v[c] . (x - pos[v]) )
 *                  gradient_c(x) = (1 / k) sum_v g_v[c]
 *   weights    both are linear in phi, with the same weights for the three channels.  Per vertex v, with A = An[v] / rn[v] (row
 *              r divided by rn[v, r]) and z_a the solution of A^T z_a = e_a, a = 0, 1: stencil entry s = x_rowptr[v] ..
 *              x_rowptr[v + 1] - 1 adds t_a = (z_a . (x_B[s] / rn[v])) / k to the d/dx_a weight of node x_out[s] and -t_a to that
 *              of v; the value weight is 1 / k on v, plus (x - pos[v]) . (the two gradient weights) on every node they touch.
 *              Entries of one node are merged (a node reached through several vertices' stencils, a stencil that names a node
 *              twice), in a fixed order.
 *   pw_ptr     int32 [P + 1]: the entries of probe p are pw_ptr[p] .. pw_ptr[p + 1] - 1 (a probe may have none: its row is zero)
 *   pw_node    int32 [nnz]: the nodes, ascending and unique within a probe
 *   pw_w       double [nnz, 3], 8-byte aligned: (value weight, d/dx weight, d/dy weight)
 *   hist       double [keep, P, GFV_PROBE_SUMS], 8-byte aligned: row n % keep; of probe p the nine doubles q = 3 c + j,
 *              j = 0 the value, 1 d/dx, 2 d/dy of channel c
 *   hist_clock int32 [keep]: the clock of a row
 * The rule: the window's, with rec and *clock as the launch finds them.
 *   take false:  no word of hist or hist_clock moves
 *   take true:   one wave per probe; lane l takes the entries e = pw_ptr[p] + l, + l + 64, ... in ascending order and, starting
 *                from +0.0, adds pw_w[e, j] * phi_c(pw_node[e]) into nine doubles - each product and each sum ONE IEEE double
 *                operation, nothing contracted; the 64 lane sums fold by the xor butterfly 32, 16, ... 1 (csrc/gfv_reduce.h);
 *                hist[n % keep, p, q] = the sum;  hist_clock[n % keep] = c
 * No floating-point atomics, nothing handed between workgroups, an order that does not depend on the grid: the same inputs give
 * the same bits.  Nothing but hist, hist_clock and rec is written.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer, P < 1, keep < 1, an x_backup that is not 16-byte aligned, or a pw_w or hist
 * that is not 8-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_PROBE_RECORD 8 /* = GFV_WINDOW_RECORD */
#define GFV_PROBE_SUMS 9
int gfv_probe_sample(const float* x_backup, const float* uvp_dim, const int32_t* batch, const int32_t* pw_ptr,
                     const int32_t* pw_node, const double* pw_w, int32_t P, const int32_t* clock, int32_t* rec, double* hist,
                     int32_t* hist_clock, int32_t keep, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Flow integrals (gfv/integrals.py): per graph the area, the kinetic energy, the enstrophy, the L2 and the max norm
 * of the discrete divergence, the peak vorticity, the circulation, the pressure integral and the flux through the inflow, the
 * outflow and the other boundary faces, for the field a run has just written; optionally the cell vorticity and the cell
 * divergence of that field.  ONE launch behind the launch that has advanced the field (gfv_rollout_advance, gfv_march_advance), on
 * the same stream.  `x_backup` and `uvp_dim` are gfv_wall_force_grad's; `clock` and `rec` are the clock and the window's record
 * (GFV_WINDOW_RECORD, above).  No gradient and no LU: every quantity is a closed-polygon sum over the plan's incidence tables.
 *   crow int32 [C + 1], kface, knode int32 [Sg], kS float [Sg, 2]: the (cell, face) incidences of cell C are k = crow[C] ..
 *              crow[C + 1] - 1; the face, the vertex and the cell's OUTWARD surface vector of incidence k
 *   es, er int32 [E]: a face's end nodes;  area float [C]: the cells' areas
 *   btype      int32 [Sg], built once on the host: 0 where the face kface[k] has two incidences; where it has exactly one: 1 if
 *              its face type is INFLOW (1), 2 if OUTFLOW (2), 3 otherwise
 *   cchunk_beg, cchunk_end int32 [n_cchunks], gcchunk_ptr int32 [B + 1]: chunks of at most GFV_FLOW_CHUNK consecutive cells that
 *              never cross a graph, and each graph's range of chunks (the form of a plan's chunk tables)
 *   partial    double [n_cchunks, GFV_FLOW_SUMS + GFV_FLOW_MAXS], 8-byte aligned: workspace
 *   hist       double [keep, B, GFV_FLOW_SUMS + GFV_FLOW_MAXS], 8-byte aligned: the twelve columns per graph, row n % keep
 *   hist_clock int32 [keep]: the clock of a row
 *   cell_out   double [C, 2], 8-byte aligned, or NULL: (Gamma_C / a, D_C / a), the cell vorticity and the cell divergence
 * The rule: the window's, with rec and *clock as the launch finds them.
 *   take false:  no word of partial, hist, hist_clock or cell_out moves
 *   take true:
 *     phi_c(i) = x_backup[i, c] / uvp_dim[3 batch[i] + c], c = u, v, p: ONE fp32 division, then double (a cell's nodes lie in the
 *     cell's graph b, the graph of its chunk: the launch reads uvp_dim[3 b + c]).  Everything below is one IEEE double operation in
 *     the order written, nothing contracted.
 *     per cell C with its n incidences k, ascending:  f = kface[k], s = es[f], r = er[f], S = (double)kS[k]
 *       u_f = 0.5 * (u_s + u_r), v_f likewise            (the trapezoid face value: exact for a linear field; NOT the residual's
 *                                                         reconstructed face value)
 *       d_k = u_f * S.x + v_f * S.y                       g_k = v_f * S.x - u_f * S.y
 *       D_C = sum_k d_k, Gamma_C = sum_k g_k, from +0.0   (the integral of div u over the cell; its circulation, the integral of
 *                                                         omega = dv/dx - du/dy)
 *       ubar, vbar, pbar = (sum_k phi(knode[k]), from +0.0) / (double)n;    a = (double)area[C]
 *     the twelve columns, per cell:
 *       0 area                a                                    6 pressure . area     pbar * a
 *       1 kinetic energy      (0.5 * (ubar*ubar + vbar*vbar)) * a  7 inflow flux         sum of d_k over btype[k] == 1, from +0.0
 *       2 enstrophy           (0.5 * (Gamma_C * Gamma_C)) / a      8 outflow flux        ... btype[k] == 2
 *       3 div^2               (D_C * D_C) / a                      9 other boundary flux ... btype[k] == 3
 *       4 net outflow         D_C                                 10 max |div|           fabs(D_C) / a
 *       5 circulation         Gamma_C                             11 max |vorticity|     fabs(Gamma_C) / a
 *     columns 0 .. 9 are sums, 10 and 11 maxima by fmax from +0.0 (a NaN is passed over).  With exactly antisymmetric kS across
 *     every interior face, column 4 = columns 7 + 8 + 9 up to the rounding of the sums.
 *     cell_out[C] = (Gamma_C / a, D_C / a), where it is not NULL
 *     per chunk: one wave; lane l takes the cells beg + l, beg + l + 64, ... < min(end, C) in ascending order from +0.0, the 64
 *     lane values fold by the xor butterfly 32, 16, ... 1 (the maxima by the same exchanges with fmax); per graph, by the workgroup
 *     that arrives last: lane l takes the chunks c0 + l, c0 + l + 64, ... in ascending order, then the same butterfly
 *     (csrc/gfv_reduce.h states the order)
 *     hist[n % keep, b, :] = the graph's twelve columns (zero for a graph without a cell);  hist_clock[n % keep] = c
 * No floating-point atomics and no sum across graphs: the same inputs give the same bits, whatever the grid.  Nothing but partial,
 * hist, hist_clock, cell_out and rec is written.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer other than cell_out, C, B, n_cchunks or keep < 1, an x_backup that is not
 * 16-byte aligned, or a kS, partial, hist or cell_out that is not 8-byte aligned (a vector kS[k] is read as one pair).
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_FLOW_RECORD 8 /* = GFV_WINDOW_RECORD */
#define GFV_FLOW_SUMS 10
#define GFV_FLOW_MAXS 2
#define GFV_FLOW_CHUNK 64
int gfv_flow_integrals(const float* x_backup, const float* uvp_dim, const int32_t* crow, const int32_t* kface,
                       const int32_t* knode, const float* kS, const int32_t* btype, const int32_t* es, const int32_t* er,
                       const float* area, const int32_t* cchunk_beg, const int32_t* cchunk_end, const int32_t* gcchunk_ptr,
                       int32_t n_cchunks, int32_t C, int32_t B, const int32_t* clock, int32_t* rec, double* partial, double* hist,
                       int32_t* hist_clock, int32_t keep, double* cell_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Learning-rate schedules evaluated on the device (gfv/schedule.py; the reference's utils/scheduler.py attached
 * at pre_train_Adam.py:203 and solve_with_grad_GPU.py:197, and torch.optim.lr_scheduler.ReduceLROnPlateau).  ONE launch of one
 * wave recomputes the rate from a device record and writes it where the Adam launches read it:
 *   hyper[0] = (float)lr                        (the 8 floats of gfv_adam_step_dev; no other word is touched)
 *   group row k, word 0 = (float)(lr * scales[k])   for k < n_groups: `group_table` is the table of gfv_adam_step_groups_dev
 *                                               ((GFV_MAX_PARAM_GROUPS + 2) * 8 words, row 0 its header; group k is row 1 + k),
 *                                               the product formed in double from the unrounded rate.  NULL: no groups.
 * rec: GFV_SCHED_RECORD doubles (8-byte aligned) of the caller's, addressed as 32-bit words w[] and as doubles d[]:
 *     w[0]  kind            (host)   GFV_SCHED_STEPEXP .. GFV_SCHED_PLATEAU
 *     w[1]  epoch
 *     w[2]  n_milestones    (host)   GRADUAL: 0 .. GFV_SCHED_MAX_MILESTONES
 *     w[3]  num_bad                  PLATEAU: epochs without improvement
 *     w[4]  cooldown_left            PLATEAU
 *     w[5]  patience        (host)   PLATEAU
 *     w[6]  cooldown        (host)   PLATEAU
 *     w[7]  warmup_epochs   (host)   PLATEAU: 0 = no warm-up
 *     w[8]  steplr_milestone (host)  STEPEXP
 *     w[9]  explr_milestone (host)   STEPEXP
 *     w[10] total_epoch     (host)   STEPEXP, GRADUAL
 *     w[11] follow_cap      (host)   FOLLOW: the largest epoch it sets; negative: none
 *     w[12..15]                      zero
 *     d[8]  lr                       the current unrounded rate
 *     d[9]  base_lr         (host)
 *     d[10] min_lr          (host)
 *     d[11] gamma           (host)   STEPEXP: steplr_gamma; EXP, GRADUAL: gamma
 *     d[12] expgamma        (host)   STEPEXP: explr_gamma; GRADUAL: expgamma
 *     d[13] decay_steps     (host)   STEPEXP: total_epoch - explr_milestone
 *     d[14] startlr         (host)   STEPEXP
 *     d[15] best                     PLATEAU: +inf at the start
 *     d[16] factor, d[17] threshold, d[18] eps, d[19] multiplier   (host)   PLATEAU
 *     w[40..47] milestones  (host)   GRADUAL, int32
 *   Words marked (host) are written by the host only; the others by the kernel (and by the host when a state is loaded).
 * mode, with the record AS THE LAUNCH FINDS IT:
 *   GFV_SCHED_EVAL    epoch unchanged; the rate is recomputed and written out.  Idempotent: for after the host has rewritten hyper
 *                     or the group table for another reason.
 *   GFV_SCHED_TICK    epoch += 1, then as EVAL - the host's lr_scheduler.step().  PLATEAU past its warm-up observes *metric first.
 *   GFV_SCHED_FOLLOW  c = *counter (a 32-bit word, e.g. word [6] `level` of gfv_march_advance's record), c = min(c, follow_cap)
 *                     when follow_cap >= 0; epoch = c if it differs; then as EVAL.  PLATEAU: as EVAL (there is no metric).
 * The rate of epoch e, every operation one IEEE double operation in the order written (pow is the device library's):
 *   STEPEXP   e < steplr_milestone: startlr;  e < explr_milestone: startlr * gamma;
 *             else min_lr + max(base_lr * gamma - min_lr, 0) * pow(expgamma, (e - explr_milestone) / decay_steps)
 *   EXP       min_lr + max(base_lr - min_lr, 0) * pow(gamma, e / decay_steps)
 *   GRADUAL   hit = the number of milestones <= min(e, total_epoch);  s = base_lr * pow(gamma, hit);
 *             e <= total_epoch: s;  else min_lr + max(s - min_lr, 0) * pow(expgamma, (e - total_epoch) / decay_steps)
 *   TABLE     table[min(max(e, 0), table_len - 1)] - a device array of doubles; without a table the rate stays
 *   PLATEAU   0 < e <= warmup_epochs: base_lr * (e / warmup_epochs) if multiplier == 1, else
 *             base_lr * ((multiplier - 1) * e / warmup_epochs + 1); nothing is observed.  Otherwise the rate stays, and a TICK
 *             observes a = (double)*metric as ReduceLROnPlateau(mode "min", threshold_mode "rel") does:
 *             a < best * (1 - threshold) ? (best = a, num_bad = 0) : num_bad += 1  (a NaN compares false: a bad epoch);
 *             cooldown_left > 0: cooldown_left -= 1, num_bad = 0;
 *             num_bad > patience: n = max(lr * factor, min_lr); lr - n > eps: lr = n;  cooldown_left = cooldown; num_bad = 0.
 *             A TICK with metric NULL observes nothing.
 * GFV_ERR_ARG (nothing launched) on rec or hyper NULL, a rec that is not 8-byte aligned, an unknown mode, FOLLOW without counter,
 * n_groups outside [0, GFV_MAX_PARAM_GROUPS], group_table with n_groups > 0 and scales NULL, table_len < 0 or table_len > 0 with
 * table NULL.  The kind is the record's: the entry point cannot read it.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_SCHED_RECORD 32
#define GFV_SCHED_MAX_MILESTONES 8
#define GFV_SCHED_EVAL 0
#define GFV_SCHED_TICK 1
#define GFV_SCHED_FOLLOW 2
#define GFV_SCHED_STEPEXP 1
#define GFV_SCHED_EXP 2
#define GFV_SCHED_GRADUAL 3
#define GFV_SCHED_TABLE 4
#define GFV_SCHED_PLATEAU 5
int gfv_lr_schedule(double* rec, int32_t mode, float* hyper, float* group_table, const double* scales, int32_t n_groups,
                    const double* table, int32_t table_len, const float* metric, const int32_t* counter, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Loss balancing: the three residual weights adapted on the device (gfv/balance.py).  The objective is
 * mean_b log(w_press * press_b + w_cont * cont_b + w_mom * (mom_x_b + mom_y_b)); the reference ships the weights as constants
 * (utils/get_param.py:59-61).  Here they live in hyper[5..7] (w_cont, w_mom, w_press: what the loss launch, its gradient and the
 * march read), and ONE launch of one wave per training step, BEHIND that step's optimiser launches, observes the step's terms and
 * may write new weights there for the NEXT step.  Classes k = 0, 1, 2: cont, mom, press - the order of hyper[5], hyper[6], hyper[7].
 *
 * losses: [B, 4] fp32 (cont, mom_x, mom_y, press) of the step, B >= 1.  The statistic of a launch, all in double:
 *   t_0(b) = (double)losses[b,0];  t_1(b) = (double)losses[b,1] + (double)losses[b,2];  t_2(b) = (double)losses[b,3]
 *   s_k = (sum_b t_k(b)) / (double)B, the sum in this fixed order, whatever the launch geometry: GFV_BALANCE_LANES = 64 partial
 *   sums, p_j = t_k(j) + t_k(j + 64) + t_k(j + 128) + ... added from the left starting at 0.0 (a j without a graph: 0.0); then
 *   for h = 32, 16, 8, 4, 2, 1:  p_j = p_j + p_(j+h) for j < h;  the sum is p_0.  No floating-point atomics.
 * rec: GFV_BALANCE_RECORD doubles (8-byte aligned) of the caller's, addressed as 32-bit words w[] and as doubles d[]:
 *     w[0]  kind            (host)   GFV_BALANCE_INVERSE or GFV_BALANCE_PROGRESS
 *     w[1]  warmup          (host)   observations before the first publish, >= 0
 *     w[2]  every           (host)   publish behind every `every`-th applied step, >= 1 (below 1: taken as 1)
 *     w[3]  n                        observations accepted
 *     w[4]  n_applied                accepted observations behind an applied step
 *     w[5]  n_updates                publishes
 *     w[6]  n_skipped                observations rejected
 *     w[7]                           zero
 *     d[4]  decay           (host)   of the moving average, in [0, 1)
 *     d[5]  floor           (host)   > 0
 *     d[6]  alpha           (host)   PROGRESS: in [0, 1)
 *     d[7]  tau             (host)   PROGRESS: > 0
 *     d[8..10]  g           (host)   INVERSE: the shares, each > 0
 *     d[11..13] w0          (host)   the base weights
 *     d[14] power                    decay^n, 1 at the start
 *     d[15..17] m                    the moving average, 0 at the start
 *     d[18..20] s                    the last accepted statistic
 *     d[21..23] s_ref                the reference statistic
 *     d[24..26] lam                  the multipliers, 1 at the start
 *     d[27..29] w                    the current weights, w0 at the start
 *     d[30..31]                      zero
 *   Words marked (host) are written by the host only; the others by the kernel (and by the host when a state is loaded).
 * The rule, with the record AS THE LAUNCH FINDS IT; every operation is one IEEE double operation in the order written (the unit is
 * built without contraction; exp is the device library's):
 *   1. s as above.  If any s_k is NaN, infinite or negative: n_skipped += 1, nothing else changes, hyper is not written.
 *   2. n += 1;  m_k = decay * m_k + (1 - decay) * s_k;  power = power * decay;  mh_k = m_k / (1 - power)  (decay == 0: mh = s);
 *      at n == 1: s_ref = mh.
 *   3. applied = hold == NULL or *hold != 0.  hold is word [3] `apply` of the accumulation record of gfv_grad_accum_dev, the word
 *      the guard, Adam and log launches read.  If applied: n_applied += 1.
 *   4. A publish happens if applied and n > warmup and n_applied % every == 0:
 *      INVERSE   R0 = (w0_0 * mh_0 + w0_1 * mh_1) + w0_2 * mh_2;  G = (g_0 + g_1) + g_2;
 *                w_k = ((g_k / G) * R0) / max(mh_k, floor).
 *                Every class then contributes its share g_k / G of the residual R0 that the base weights would give.
 *      PROGRESS  rho_k = mh_k / max(s_ref_k, floor);  z_k = rho_k / tau;  zm = max(z_0, z_1, z_2);  e_k = exp(z_k - zm);
 *                E = (e_0 + e_1) + e_2;  lh_k = 3 * (e_k / E);  lam_k = alpha * lam_k + (1 - alpha) * lh_k;  w_k = w0_k * lam_k;
 *                s_ref = mh.  (ReLoBRaLo of Bischof and Kraus without its random look-back: a term that falls more slowly than
 *                the others gains weight; the sum of lam stays 3.)
 *      then hyper[5 + k] = (float)w_k, the record's w = w, n_updates += 1.  No other word of hyper is touched.
 * One wave: every lane loads the record, the hold word and its share of losses; all loads stand in front of all stores in program
 * order; lane 0 writes the record and hyper with ordinary vector stores.  No atomics, no arrival counter.
 * GFV_ERR_ARG (nothing launched) on losses, rec or hyper NULL, B < 1, a rec that is not 8-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_BALANCE_RECORD 32
#define GFV_BALANCE_LANES 64
#define GFV_BALANCE_INVERSE 1
#define GFV_BALANCE_PROGRESS 2
int gfv_loss_balance(const float* losses, int32_t B, double* rec, float* hyper, const int32_t* hold_or_null, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Observation term: measured fields beside the PDE residual (gfv/observe.py, DESIGN.md 5s, csrc/obs.hip).  The objective becomes
 *   mean_b log(w_press * press_b + w_cont * cont_b + w_mom * (mom_x_b + mom_y_b) + w_obs * obs_b).
 * What is fitted is the network's OWN nodal prediction, phi[:, 0:3] = BC(10 tanh(dec / 10)) (gfv_phi_fwd), before the
 * cell-to-node smoothing, in the units of the returned uvp_node.  For node i of graph b and channel c in (u, v, p):
 *   pred = (phi[i, c] * uvp_dim[b, c]) * sigma[b, c]       fp32, the order of gfv_cell_to_node
 *   e    = pred - target[i, c]                             fp32
 *   w    = weight[i, c] >= 0                               fp32; an element with w == 0 is skipped BEFORE its target is read into
 *                                                          any arithmetic: unobserved targets may hold anything, NaN included
 *   S_b  = sum w * (e * e),  W_b = sum w                   every product and sum in double; per row ((c0 + c1) + c2); per chunk and
 *                                                          per graph in the fixed order of gfv_rollout_advance (csrc/gfv_reduce.h)
 *   obs_b = (float)(S_b / W_b), 0 when W_b == 0            divided in double, rounded once
 *
 * gfv_obs_fwd: ONE launch behind the forward (one wave per chunk).  partial_ws: 2 doubles per chunk, (S, W); counter: one int32,
 *   zero before the first launch and left at zero (write-through arrival, csrc/gfv_reduce.h).  The workgroup that arrives last
 *   writes, with the arithmetic of gfv_fvm_fwd_tail's loss (fp32, 64 strided partial sums of logf folded from the left):
 *     tot_b = (w_press * press_b + w_cont * cont_b + w_mom * mom_x_b + w_mom * mom_y_b) + w_obs * obs_b      hyper[5..7], *w_obs
 *     loss[0] = (sum_b logf(tot_b)) / B;  inv_b = 1 / (tot_b * B);  gloss[b] = (w_cont, w_mom, w_mom, w_press) * inv_b
 *     rec[b] = (obs_b, (float)W_b, gobs_b = w_obs * inv_b, tot_b)                          GFV_OBS_RECORD floats per graph
 *   loss and gloss are OVERWRITTEN: the launch stands behind the one that formed them from `losses` alone.  w_obs is one device
 *   float of the caller's: a new value reaches recorded and captured launches without re-recording.
 * gfv_obs_bwd: ONE launch, one thread per node, between gfv_fvm_bwd_fused / gfv_phi_bwd and the decoder's backward:
 *     g_dec[i, c] += gobs_b * (2 * w * e * (uvp_dim[b, c] * sigma[b, c]) / W_b) * (1 - tanhf(dec[i, c] / 10)^2)       fp32
 *   where w != 0 and gfv_phi_bwd lets gradient through (u, v: not at WALL / INFLOW / PRESS / INWALL nodes; p: not at PRESS
 *   nodes).  No other element is written: with every weight zero g_dec keeps its bits.
 * gfv_obs_gather: ONE launch (pool path): dst_values / dst_weights [dst_rows, 3] rows off_b .. off_b + rows[b] - 1 (off = the
 *   running sum of rows) = values[b] / weights[b] [rows[b], 3]; a graph with values[b] == weights[b] == NULL gets zero weights and
 *   its values are left alone.  values, weights and rows are HOST arrays of B entries (device addresses, row counts): they travel
 *   by value in the launch's argument block, so the launch is issued per batch and is never part of a recorded list.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer, B outside [1, GFV_POOL_MAX_GRAPHS], N or n_chunks < 1 (gfv_obs_bwd: N < 0;
 * N == 0 launches nothing), a phi or rec that is not 16-byte aligned, a negative row count, only one of values[b] / weights[b]
 * NULL, or rows that sum to more than dst_rows.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_OBS_RECORD 4
int gfv_obs_fwd(const float* phi, const float* target, const float* weight, int32_t N, const int32_t* chunk_beg,
                const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, const float* uvp_dim,
                const float* sigma, const float* losses, const float* hyper, const float* w_obs, double* partial_ws,
                int32_t* counter, float* rec, float* loss, float* gloss, void* stream);
int gfv_obs_bwd(const float* rec, const float* dec, const float* phi, const float* target, const float* weight,
                const int32_t* batch, const int32_t* node_type, const float* uvp_dim, const float* sigma, int32_t N, int32_t B,
                float* g_dec, void* stream);
int gfv_obs_gather(const float* const* values, const float* const* weights, const int32_t* rows, int32_t B, float* dst_values,
                   float* dst_weights, int64_t dst_rows, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation over a device pool (gfv/evaluate.py; the training objective of pre_train_Adam.py:177-184 and field errors on
 * entries that are not trained on).  ONE launch behind the forward-only step of a batch turns its outputs into a record of
 * GFV_EVAL_RECORD floats per graph and writes it to row entry[b] of table [n_entries, GFV_EVAL_RECORD]:
 *   columns 0-3    losses[b, 0:4] (cont, mom_x, mom_y, press), bit copies
 *           4-6    || pred - cur ||_2 per channel u, v, p: pred = uvp_node, cur = x_raw[:, 0:3] (the entry's own state)
 *           7-9    || pred ||_2 per channel
 *           10-12  || pred - tgt ||_2 per channel, tgt = target3;  NaN for a graph with has_target[b] == 0
 *           13-15  || tgt ||_2 per channel;                        NaN likewise
 * over the nodes of graph b (chunk_beg / chunk_end / gchunk_ptr as for gfv_rollout_advance).  Nothing else is written: x_raw, the
 * batch and the pool stay as they are.  entry and has_target are HOST arrays of B int32; they travel by value in the launch's
 * argument block (as the indices of gfv_pool_assemble), so the launch is issued per batch and is not part of a recorded list.
 * target3 [N, 3] is indexed like uvp_node and read only over the graphs that have a target; it may be NULL when none has.
 * partial_ws: GFV_EVAL_RECORD - 4 doubles per chunk; counter: one int32, zero before the first launch and left at zero.
 * Differences in fp32, squares and sums in double in the fixed order of gfv_rollout_advance, the square root in double, rounded
 * to fp32: no floating-point atomics, results identical run to run.
 * GFV_ERR_ARG (nothing launched) on a NULL pointer (target3: only with a target flag set), N, n_chunks, B or n_entries < 1,
 * B > GFV_POOL_MAX_GRAPHS, an entry outside [0, n_entries), the same entry twice or an x_raw that is not 16-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_EVAL_RECORD 16
int gfv_eval_collect(const float* uvp_node, const float* x_raw, const float* target3, int32_t N, const int32_t* chunk_beg,
                     const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, const float* losses,
                     const int32_t* entry, const int32_t* has_target, float* table, int32_t n_entries, double* partial_ws,
                     int32_t* counter, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training log (gfv/trainlog.py): per-step losses, norms and guard decisions kept on the device.  Two launches,
 * issued in this order behind the optimiser launches of a step (so every record they read is the one Adam left), eagerly in
 * every launch mode and never inside a recorded list or a captured graph; the host reads the ring once per epoch.
 *
 * gfv_train_log_norms: ONE launch.  For each of K buckets: sum of g[i]^2, sum of p[i]^2 and the count of non-finite g[i] over
 *   the bucket's elements, three doubles into sums [K, 3].  g is read as stored (no grad_scale, no clip coefficient).
 *   segs: DEVICE table of (offset, count) int64 pairs into g and p, the format of the guard's table; bucket k owns the segments
 *   bucket_tab[k][0] .. bucket_tab[k][1] - 1.  bucket_tab: DEVICE int64 [K, 4] = {first segment, one past the last segment,
 *   first chunk, elements}: elements = the sum of the bucket's counts (at least 1), chunks are GFV_TRAIN_LOG_CHUNK logical
 *   elements of one bucket, numbered bucket after bucket (first chunk of k + 1 = first chunk of k + its chunk count, what
 *   gfv_train_log_chunks says of its element count); n_chunks = their total.  Nothing outside a segment is read.
 *   Squares and sums in double, in a FIXED order defined over the logical index j of a bucket's concatenated elements - not over
 *   the grid, timing or a segment's alignment - with no floating-point atomics:
 *     chunk c of a bucket = elements 1024 c .. min(1024 (c + 1), n) - 1; lane l of one wave adds, from +0.0, the elements
 *     1024 c + 256 r + 4 l + (0 .. 3) for r = 0 .. 3 in ascending order; the 64 lanes fold by xor butterfly, levels 32 .. 1;
 *     the workgroup that arrives last folds a bucket's chunk sums: lane l adds chunks l, l + 64, ... ascending, same butterfly.
 *   16-byte loads where four consecutive logical elements lie in one segment at a 16-byte aligned address, element loads
 *   elsewhere: the same values in the same order.
 *   workspace: gfv_train_log_workspace_bytes of n_chunks, 8-byte aligned, ZEROED once by the caller (first word: the arrival
 *   counter, left at zero by every launch).  K == 0: GFV_OK, nothing launched, nothing written.
 *   GFV_ERR_ARG (nothing launched) on K < 0 or above GFV_TRAIN_LOG_MAX_BUCKETS and, with K > 0, a NULL pointer (a NULL bucket
 *   table included), n_chunks < 1 or a misaligned workspace.
 *
 * gfv_train_log_append: ONE workgroup.  Writes row (cursor mod capacity) of the ring and then cursor += 1; cursor is a DEVICE
 *   64-bit count of all appends.  A row is gfv_train_log_row_words of (max_graphs, K) 32-bit words:
 *     [0..1]  ordinal (int64)     the cursor before this append
 *     [2]     adam_t              state[0]: optimiser steps completed, this one included
 *     [3]     loss                loss[0], bit copy
 *     [4]     lr                  hyper[0]
 *     [5]     B (int32)           graph count of this call
 *     [6] [7] [8]                 guard[2] norm, guard[3] coef, guard[4] decision (int32); guard == NULL: NaN, 1.0f, 0
 *     [9]     apply (int32)       accum[3]; accum == NULL: 1
 *     [10]    applied (int32)     1 if apply and the decision carries no skip bit, else 0
 *     [11..15]                    zero
 *     [16 .. 16 + 4 max_graphs)   terms: losses[B, 4] bit copies, rows B and beyond zero
 *     then max_graphs int32       entries: the pool entry of every slot, -1 where there is none
 *     (one zero word if 5 max_graphs is odd) then K x 3 doubles: sums of the norms launch
 *   entry: HOST array of B int32 or NULL (none: every slot -1); it travels by value in the launch's argument block.
 *   table: optional DEVICE int32 [n_entries, GFV_TRAIN_LOG_ENTRY_RECORD], updated for slot 0, 1, .. B - 1 in this order for every
 *   entry >= 0 (the same entry twice counts two visits, the later slot's terms stay):
 *     [0] visits (int32)  [1] ordinal of the last visit (int32, the low word)  [2..5] the four terms of the last visit  [6] [7] zero
 *   GFV_ERR_ARG (nothing launched) on a NULL ring, cursor, state, hyper, loss or losses, capacity < 1, B outside [1, max_graphs],
 *   max_graphs above GFV_POOL_MAX_GRAPHS, an entry outside [-1, n_entries) (without a table: below -1), K < 0 or above
 *   GFV_TRAIN_LOG_MAX_BUCKETS, NULL sums with K > 0, a table with n_entries < 1, a ring or cursor that is not 8-byte aligned.
 * gfv_train_log_row_words: GFV_ERR_ARG for a max_graphs outside [1, GFV_POOL_MAX_GRAPHS] or a K outside the range above.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_TRAIN_LOG_CHUNK 1024
#define GFV_TRAIN_LOG_HEAD 16
#define GFV_TRAIN_LOG_ENTRY_RECORD 8
#define GFV_TRAIN_LOG_MAX_BUCKETS 32
int64_t gfv_train_log_chunks(int64_t n_elems);
size_t gfv_train_log_workspace_bytes(int64_t n_chunks);
int32_t gfv_train_log_row_words(int32_t max_graphs, int32_t K);
int gfv_train_log_norms(const float* g, const float* p, const int64_t* segs, const int64_t* bucket_tab, int32_t K, int64_t n_chunks,
                        double* sums, void* workspace, void* stream);
int gfv_train_log_append(void* ring, int32_t capacity, int32_t max_graphs, int32_t K, int64_t* cursor, const float* state,
                         const float* hyper, const float* loss, const float* losses, int32_t B, const float* guard,
                         const float* accum, const int32_t* entry, const double* sums, int32_t* table, int32_t n_entries,
                         void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Anderson acceleration AA(m) of the steady-state rollout (gfv/anderson.py, gfv/rollout.py): two launches between
 * the forward-only step and gfv_rollout_advance.  Per graph b over its node rows x 3 channels, fp32: x = x_backup[:, 0:3],
 * g = uvp_node, f = g - x.  State of the caller's, zero before the first step and never touched by anything else:
 *   f_prev, g_prev [N, 3] float;  dF, dG [m, N, 3] float (ring columns);  aa_state [B, 4] int32 (valid columns cnt, ring head,
 *   has_prev, restarts);  r_prev [B] double (the last || f ||);  gamma [B, GFV_AA_MAX_DEPTH] double;  partial_ws
 *   GFV_AA_PARTIALS * n_chunks doubles;  counter one int32 (left at zero);  aa_table [K_max, B, 4] float.
 * gfv_anderson_gram: per row, with has_prev: dF[head] = f - f_prev, dG[head] = g - g_prev (fp32); then f_prev = f, g_prev = g.
 *   Over the mk = min(cnt + has_prev, m) valid columns, the new one included, in double and in the fixed order of
 *   gfv_rollout_advance (no floating-point atomics; a graph's sums do not depend on the rest of the batch): the upper triangle of
 *   A = dF^T dF, dF^T f, || f ||^2, || g ||^2.  Then, per graph, with k = *step (the rollout's step counter, not written here), in
 *   this order:
 *     1. || f ||^2 not finite: restart - cnt = 0, has_prev = 0, flag GFV_AA_NONFINITE;
 *     2. has_prev, restart > 0 and || f || > restart * r_prev: restart - cnt = 0 (the pair is kept), flag GFV_AA_GROWTH;
 *     3. mk == 0 or k < start: depth 0 (the column is kept: cnt = mk, the head advances);
 *     4. (A + reg * trace(A) / mk * I) gamma = dF^T f by Cholesky in double; a pivot <= 0 (an all-zero Gram matrix included) or a
 *        gamma that is not finite: restart - cnt = 0, flag GFV_AA_SINGULAR;
 *     5. otherwise depth = mk, cnt = mk, the head advances.
 *   Every restart adds one to aa_state[b, 3].  gamma[b] is written in ring-slot order, zero for unused slots and whenever the
 *   depth is 0; aa_table[k, b] = (|| f ||, || g ||, depth, flags).  With k outside [0, K_max) nothing is decided or mixed.
 * gfv_anderson_mix: over the rows of every graph with depth > 0 (aa_table[k, b, 2]), in place,
 *     uvp_node = g - (1 - beta) f - sum_j gamma_j (dG_j - (1 - beta) dF_j)
 *   with f_cur = this step's f (what the gram launch left in f_prev), j in ascending ring slot over the slots with gamma_j != 0,
 *   in double, rounded to fp32 once.  Rows of a graph with depth 0 are not written.  A row whose g never changes (dG = 0, f = 0)
 *   keeps its bits.
 * Both return GFV_ERR_ARG - before anything touches a device, nothing launched - on a NULL pointer, N, n_chunks, B or K_max < 1,
 * m outside 1 .. GFV_AA_MAX_DEPTH, beta outside (0, 1], reg negative or NaN, restart negative, NaN or in (0, 1] (0 switches the
 * growth test off), or a double buffer that is not 8-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_AA_MAX_DEPTH 8
#define GFV_AA_PARTIALS 46   /* 36 (upper triangle) + 8 (dF^T f) + || f ||^2 + || g ||^2 */
#define GFV_AA_NONFINITE 1
#define GFV_AA_GROWTH 2
#define GFV_AA_SINGULAR 4
int gfv_anderson_gram(const float* uvp_node, const float* x_backup, int32_t N, const int32_t* chunk_beg, const int32_t* chunk_end,
                      const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, int32_t m, double reg, double restart, int32_t start,
                      float* f_prev, float* g_prev, float* dF, float* dG, int32_t* aa_state, double* r_prev, double* gamma,
                      double* partial_ws, int32_t* counter, float* aa_table, int32_t K_max, const int32_t* step, void* stream);
int gfv_anderson_mix(float* uvp_node, const float* f_cur, int32_t N, const int32_t* chunk_beg, const int32_t* chunk_end,
                     const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, int32_t m, double beta, const float* dF,
                     const float* dG, const double* gamma, const float* aa_table, int32_t K_max, const int32_t* step, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Anderson acceleration per slot of a sweep (gfv/sweep.py `Sweep(..., anderson=m)`, gfv/anderson.py SlotAndersonState; DESIGN.md
 * 5e, 5k): the SLOT form of the two launches above, between the forward-only step and gfv_sweep_advance_aa.  The arithmetic, the
 * summation order, the decision and the mix are those of gfv_anderson_gram / gfv_anderson_mix (one shared kernel body,
 * csrc/anderson_kernel.h); what differs:
 *   rings      a ring row of node i of slot b is  b * ring_stride + (i - chunk_beg[gchunk_ptr[b]])  - the node's index inside its
 *              own graph, in the slot's own region: f_prev, g_prev [B * ring_stride, 3], dF, dG [m][B * ring_stride, 3].  A swap
 *              of a neighbour to an entry of another size moves nothing under a live slot's columns.  ring_stride >= the node
 *              count of every graph that ever runs (the host checks; a node beyond it is not touched).
 *   step index the k compared with `start` is the slot's own age, slots[b, 0] (gfv_sweep_advance_aa increments it afterwards).
 *   frozen     a slot with slots[b, 2] (done) != 0 when the launch starts is skipped entirely: none of its rings, state words,
 *              gamma or records changes, and the mix writes none of its rows.
 *   below tol  after decisions 1 and 2: when the fp32 quotient (float)|| f || / (float)|| g || - formed exactly as
 *              gfv_sweep_advance_aa forms rel - is below ctl.tol (ctl: the 16 bytes of gfv_sweep_advance), the depth is 0 and the
 *              column is kept.  A step that can latch therefore always advances to the model's own output G(x_k).
 *   records    aa_slot [B, 4] float = (|| f ||, || g ||, depth, flags) of the slot's last live step (it stands where
 *              aa_table[k, b] stands above; the mix reads its depth);  aa_count [B, 4] int32 += (depth > 0, NONFINITE, GROWTH,
 *              SINGULAR) per live step.  The host zeroes aa_state[b], r_prev[b] and aa_count[b] when slot b takes a new entry;
 *              rings need no clearing (cnt = 0 and has_prev = 0 mask them; stale values, NaN included, are never read).
 * gfv_sweep_advance_aa is gfv_sweep_advance with rel = aa_slot[b, 0] / aa_slot[b, 1] (the true fixed-point residual
 * || G(x) - x || / || G(x) ||, not the norm of the possibly mixed update it applied) and last[b, 4:6] = those two values;
 * age, streak, patience, min / max steps, freeze, state3 and the mirror are as there.  partial_ws is not used by it but must be
 * given (one signature, one check).
 * GFV_ERR_ARG - before anything touches a device, nothing launched - as for the rollout form, and on ring_stride < 1.
 * ---------------------------------------------------------------------------------------------------------- */
int gfv_sweep_anderson_gram(const float* uvp_node, const float* x_backup, int32_t N, const int32_t* chunk_beg,
                            const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, int32_t m, double reg,
                            double restart, int32_t start, int32_t ring_stride, float* f_prev, float* g_prev, float* dF, float* dG,
                            int32_t* aa_state, double* r_prev, double* gamma, double* partial_ws, int32_t* counter, const void* ctl,
                            const int32_t* slots, float* aa_slot, int32_t* aa_count, void* stream);
int gfv_sweep_anderson_mix(float* uvp_node, const float* f_cur, int32_t N, const int32_t* chunk_beg, const int32_t* chunk_end,
                           const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, int32_t m, double beta, int32_t ring_stride,
                           const float* dF, const float* dG, const double* gamma, const int32_t* slots, const float* aa_slot,
                           void* stream);
int gfv_sweep_advance_aa(const float* uvp_node, float* x_backup, float* x, int32_t N, const int32_t* chunk_beg,
                         const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, const float* losses,
                         double* partial_ws, const void* ctl, int32_t* slots, float* last, float* state3, int32_t* mirror_dev,
                         int32_t* state, const float* aa_slot, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Pool training (gfv/pool.py BatchArena, gfv/pool_trainer.py; the changing-batch loop of pre_train_Adam.py:112-198 with
 * Data_Pool.payback, Graph_loader.py:370-396): a batch of ANY entries of the device-resident pool assembled into FIXED memory
 * by one launch, and the prediction written back by one launch.
 *
 * The source table, built once per pool: one row of GFV_POOL_ROW_HEAD + 2 * n_attrs int64 per entry -
 *   [n nodes, n faces, n cells, n incidences, n stencil entries, n slice chunks, 0, 0 | device pointer of every pooled attribute |
 *    32-bit words of every pooled attribute]
 * - the same bytes in host memory (argument checks, grid sizes) and in device memory (read by the kernels).  What an attribute is
 * says attr_info[a] = mode | offset kind << 4:
 *   mode GFV_POOL_COPY    words copied as they are (floats, type ids)
 *        GFV_POOL_ADD     int32 indices: the entry's words + the offset of its position in the batch
 *        GFV_POOL_ROWPTR  a CSR row pointer (rows + 1 words): all but the last word of every entry, the last word too of the
 *                         last one, + the offset of the non-zero kind
 *        GFV_POOL_FILL    no source: `words` times the position in the batch (graph id per node / cell)
 *   offset kind 0 none, 1 nodes, 2 faces, 3 2 x faces, 4 cells, 5 incidences, 6 stencil entries.
 * The offsets are formed INSIDE the launch by a prefix sum over the B entries, whose indices travel by value in the launch's
 * argument block: a buffer the host rewrites for the next step would race with a launch that is still queued.  The same launch
 * writes the small per-graph arrays: gnode_ptr, gcell_ptr, gchunk_ptr, gunit_ptr [B + 1] and chunk_beg / chunk_end (node chunks of
 * `slice_chunk` rows that never cross a graph), in small[0 .. 5] in that order.  Streaming copies: 16-byte stores always (every
 * dst[a] is 16-byte aligned), 16-byte loads where the source position allows.
 * gfv_pool_assemble returns GFV_ERR_ARG - before anything touches a device - for a NULL table or argument, B < 1, B above
 * max_graphs or GFV_POOL_MAX_GRAPHS, an index outside [0, n_entries), an attribute whose batch exceeds dst_cap_words[a], more
 * chunks than max_chunks, a misaligned destination.
 * ---------------------------------------------------------------------------------------------------------- */
#define GFV_POOL_MAX_GRAPHS 64
#define GFV_POOL_MAX_ATTRS 56
#define GFV_POOL_ROW_HEAD 8
enum { GFV_POOL_COPY = 0, GFV_POOL_ADD = 1, GFV_POOL_ROWPTR = 2, GFV_POOL_FILL = 3 };
typedef struct {
  const int64_t* table_host; /* [n_entries, GFV_POOL_ROW_HEAD + 2 * n_attrs] */
  const int64_t* table_dev;  /* the same bytes in device memory */
  int32_t n_entries, n_attrs;
  int32_t max_graphs;        /* capacity of the small per-graph arrays: max_graphs + 1 words each */
  int32_t slice_chunk;       /* nodes per chunk of chunk_beg / chunk_end */
  int64_t max_chunks;        /* capacity of chunk_beg / chunk_end */
  int32_t attr_info[GFV_POOL_MAX_ATTRS];
  void* dst[GFV_POOL_MAX_ATTRS];             /* the batched tensor of every attribute, 16-byte aligned */
  int64_t dst_cap_words[GFV_POOL_MAX_ATTRS]; /* its capacity */
  int32_t* small[6];
  int32_t B, reserved;
  int32_t idx[GFV_POOL_MAX_GRAPHS];          /* the entries of the batch, in order */
} gfv_pool_args_t;
size_t gfv_pool_args_bytes(void);                /* sizeof of the struct above as the library was compiled */
size_t gfv_pool_table_bytes(int32_t n_entries, int32_t n_attrs);
/* host-side validation of a table: sizes >= 0 and within int32, every attribute with words > 0 has a 4-byte aligned source unless
 * it is a fill, a row pointer has at least one word.  GFV_OK or GFV_ERR_ARG; touches no device. */
int gfv_pool_table_check(const int64_t* table_host, int32_t n_entries, int32_t n_attrs, const int32_t* attr_info);
int gfv_pool_assemble(const gfv_pool_args_t* args, void* stream);
/* The inverse of the assembly of the node state: rows of uvp_node [N, 3] of the batch go into columns 0 .. 2 of each entry's own
 * x [n_i, 12] - the attribute `x_attr` of the table -; raw != NULL: also into columns 0 .. 2 of raw [N, 12], the arena's
 * un-normalised state the next inner step of the same batch starts from.  An entry that appears more than once in the batch takes
 * its LAST occurrence; the earlier ones are skipped - one writer per word.  N must equal the batch's node count.
 * GFV_ERR_ARG as for gfv_pool_assemble, and for a NULL uvp_node, x_attr outside the table or a wrong N. */
int gfv_pool_payback(const int64_t* table_host, const int64_t* table_dev, int32_t n_entries, int32_t n_attrs, int32_t x_attr,
                     const int32_t* idx, int32_t B, const float* uvp_node, int64_t N, float* raw, void* stream);

/* Pool renewal (gfv/pool.py DevicePool.renew, gfv/renew.py; Data_Pool.reset_env -> transform_mesh -> init_env,
 * Graph_loader.py:154-229,389-396, Load_mesh.py:80-131, Set_BC.py:6-66): the boundary condition of K entries re-drawn and their
 * fields restarted by ONE launch.  The K records travel by value in the launch's argument block (as the indices of
 * gfv_pool_assemble).  Per node of every entry, in init_env's order: (u, v, p) from the initial-field kind over all nodes; on
 * INFLOW / IN_WALL / PRESS_POINT nodes (u, v) from the inlet kind; on WALL nodes (u, v) = 0; on IN_WALL nodes (u, v, p) halved;
 * y = (u, v) * (1.0f / (float)U) (the reciprocal product torch forms for a division by a host scalar); x[:, 0:3] = (u, v, p),
 * x[:, 3:12] = coef[0 .. 8].  One thread per entry writes theta = coef[0 .. 8], dt = coef[9], uvp_dim = coef[10 .. 12].
 * Profile kinds (evaluated in float64 on pos, rounded to fp32; no contraction):
 *   GFV_RENEW_NONE         zeros
 *   GFV_RENEW_PARABOLIC    u = (6 U (py - lo)) * (((hi - lo) - (py - lo)) / ((hi - lo) * (hi - lo))), (lo, hi) = yrange[0 .. 1] for
 *                          the initial field (all nodes), yrange[2 .. 3] for the inlet targets (inlet nodes)
 *   GFV_RENEW_UNIFORM      u = U
 *   GFV_RENEW_UNIFORM_AOA  (u, v) = (float)U * ((float)cos_aoa, (float)sin_aoa): fp32 products
 *   GFV_RENEW_TAYLOR_GREEN u = U sin(2 pi x) cos(2 pi y), v = -U cos(2 pi x) sin(2 pi y), p = -(U / 4) (cos(4 pi x) + cos(4 pi y))
 * yrange is DEVICE memory (it depends on geometry only; the caller reduces it once per topology); nothing else is read from the
 * device but pos and node_type.  No reduction, no atomics, no LDS.
 * GFV_ERR_ARG - before anything touches a device, nothing launched - on NULL records, K outside [1, GFV_POOL_MAX_GRAPHS], a NULL
 * pointer inside a record, N < 1, an unknown kind, U == 0 or not finite, or two records with the same x (two blocks would race). */
enum { GFV_RENEW_NONE = 0, GFV_RENEW_PARABOLIC = 1, GFV_RENEW_UNIFORM = 2, GFV_RENEW_UNIFORM_AOA = 3, GFV_RENEW_TAYLOR_GREEN = 4 };
typedef struct {
  float* x;                  /* [N, 12] */
  float* y;                  /* [N, 2] */
  float* theta;              /* [1, 9] */
  float* dt;                 /* [1] */
  float* uvp_dim;            /* [1, 3] */
  const int32_t* node_type;  /* [N] */
  const double* pos;         /* [N, 2] */
  const double* yrange;      /* [4]: min, max of pos[:, 1] over all nodes; min, max over the inlet nodes (+inf, -inf: none) */
  double U, cos_aoa, sin_aoa;
  float coef[13];            /* theta_PDE [9] | dt_graph | uvp_dim [3] */
  int32_t N, inlet_kind, init_kind;
} gfv_renew_rec_t;           /* gfv_struct_size(10) */
int gfv_pool_renew(const gfv_renew_rec_t* recs, int32_t K, void* stream);

/* ----------------------------------------------------------------------------------------------------------
 * L-BFGS on flat fp32 vectors (csrc/lbfgs.hip; gfv/optim.py LBFGS): torch.optim.LBFGS's two-loop recursion carried out on
 * coefficients over the basis {s slots, y slots, g} with the matrix M of their dot products - a fixed number of launches per
 * search direction whatever the history size is, and no host synchronisation while it is computed.
 *
 * Memory the caller owns, all of it 16-byte aligned, n a multiple of 4 (the flat layout of gfv.engine.GradStore):
 *   S, Y      float  [slots, n]      the ring of pairs, slots = history_size + 1 <= 129: the candidate pair always has a free
 *                                    slot, so a rejected one costs the oldest pair nothing
 *   state     int32  [8]             ring head, number of stored pairs; zero at first
 *   M         double [R, R]          R = 2 * slots + 1: row i < slots is s of slot i, slots + i is y of slot i, 2 * slots is g
 *   partial   double [gfv_lbfgs_workspace_doubles]   per-workgroup partial sums
 *   delta     double [R]             the direction's coefficients
 *   res       double [16]            result block: [0] g.d, [1] max|g|, [2] sum|g|, [3] accepted, [4] H_diag (kept from call to
 *                                    call), [5] stored pairs, [8] (its first 4 bytes) the bits of the float max|d|
 * PADDING IS NOT DATA: every vector handed in as g, d or a ring row must be zero in the padding slots of the flat layout.  The
 * padding of a flat gradient holds whatever a workspace held (see the weight-gradient launches above), so a gradient enters
 * through the masked copy of the dot launch below and nothing else.
 * mode: 0 an iteration with a candidate pair; 1 the first iteration (no pair: head, count = 0, H_diag = 1, d = -g);
 *       2 rebuilding M from ring rows a checkpoint filled (the candidate is accepted as it is, nothing else changes).
 * The launches of one direction, in order:
 *   pair      first == 0: y = g - g_prev and s = t * d into slot (head + count) % slots; always g_prev = g
 *   multidot  candidate s, candidate y and g against every stored row, the candidate's and g, + max|g|, sum|g|: per tile of
 *             4096 columns, sums in double
 *   coef      one workgroup: folds the partials in a fixed order into M; accepts the candidate if y.s > 1e-10 (torch's rule:
 *             then the ring advances and H_diag = y.s / y.y); the recursion in double; writes delta and the result block
 *   combine   d = -sum_j delta_j b_j, the sum of an element in double and rounded once; raises res[8] to max|d|
 * Same inputs, same bits: every sum has a fixed order, no floating-point atomics.  All return GFV_ERR_ARG - before anything
 * touches a device - for a NULL or misaligned pointer, slots outside [2, 129], n <= 0 or not a multiple of 4, an unknown mode.
 * ---------------------------------------------------------------------------------------------------------- */
size_t gfv_lbfgs_workspace_doubles(int32_t slots, int64_t n);   /* 0 for arguments the launches refuse */
int gfv_lbfgs_pair(float* S, float* Y, int32_t slots, int64_t n, const int32_t* state, const float* g, float* g_prev,
                   const float* d, double t, int32_t first, void* stream);
int gfv_lbfgs_multidot(const float* S, const float* Y, int32_t slots, int64_t n, const int32_t* state, const float* g,
                       double* partial_ws, int32_t mode, void* stream);
int gfv_lbfgs_coef(int32_t* state, double* M, const double* partial_ws, double* delta, double* res, int32_t slots, int64_t n,
                   int32_t mode, void* stream);
int gfv_lbfgs_combine(const float* S, const float* Y, int32_t slots, int64_t n, const int32_t* state, const float* g,
                      const double* delta, float* d, double* res, void* stream);
/* out[0] = a . b, out[1] = max|a|, out[2] = sum|a| in double, in a fixed order (per-tile partials in partial_ws [3 per 4096
 * elements], folded by the workgroup that arrives last: `counter` is an int32 the launch leaves at zero) of a MASKED a: elements
 * whose byte of `mask` (one byte per element) is 0 count as zero - by selection, so a NaN or 1e30 there does not leak -, and
 * the masked a is written to copy_out.  This is how a gradient enters the optimiser's own buffers.  Every pointer 16-byte
 * aligned. */
int gfv_lbfgs_dot(const float* a, const uint8_t* mask, float* copy_out, const float* b, int64_t n, double* partial_ws,
                  int32_t* counter, double* out, void* stream);
/* p = x0 + t * d (one fused multiply-add per element) where the mask byte is non-zero; p keeps its value elsewhere.  x0 == p
 * is allowed. */
int gfv_lbfgs_axpy(float* p, const float* x0, const float* d, double t, const uint8_t* mask, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GFV_H_ */
